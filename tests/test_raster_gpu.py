"""Polygons to label images on the GPU (csrc/raster.hip): the device route of utils.raster against the numpy form (itself checked against the plain
loops of tests/raster_ref.py without a GPU), the kernels' raw outputs through ops against those loops, the scan at its chunk borders, both paint
forms, the status word, the round trip from label_outlines and the chain to prompts_from_labels on device tensors.  Integer work: every assertion is
equality.

The crossings of closed rings come in pairs, so a crossing count is even: the combs put C at 2046 / 2048 / 2050 and the SPAN count -- what the
per-pixel paint scans -- at 2047 / 2048 / 2049 / 5 * 2048 + 77; the n-gons put the edge count there, raster_scan is called at those lengths."""
import json

import numpy as np
import pytest
import torch

from tests import raster_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BORDERS = (2047, 2048, 2049, 5 * 2048 + 77)
COMBS = (1023, 1024, 1025) + BORDERS


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def N(t):
    return t.cpu().numpy().astype(np.int64)


def run(c, **kw):
    from ullsam_amd.utils import raster as RA
    return RA.rasterize_polygons(c["vertices"], c["start"], c["ring_label"], c["size"], c["order"], c["num"], **kw)


def _same(got, want, what):
    for name, g, w in zip(got._fields, got, want):
        assert g.is_cuda and g.dtype == torch.int32 and tuple(g.shape) == tuple(w.shape) and torch.equal(g.cpu(), w), (what, name)


def _shifted(t, off):
    """the same values at a base pointer that is no multiple of 16 bytes"""
    flat = torch.zeros((t.numel() + 8,), dtype=t.dtype, device=DEV)
    flat[off:off + t.numel()] = t.reshape(-1)
    v = flat[off:off + t.numel()].view(t.shape)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


@pytest.fixture(scope="module")
def small():
    return R.cases()


@pytest.fixture(scope="module")
def inputs(small):
    out = dict(small)
    out.update(R.span_cases())
    out.update({f"{n}-gon": R.ngon(n) for n in BORDERS})
    out.update({f"comb of {s} spans": R.comb(s) for s in COMBS})
    out["one long edge next to 500 short ones"] = R.long_edge()
    return out


@pytest.fixture(scope="module")
def host(inputs):
    """{name: the numpy form's Raster}: computed once, shared, never changed."""
    return {name: run(c) for name, c in inputs.items()}


def test_device_route_equals_the_host_form(inputs, host):
    for name, c in inputs.items():
        _same(run(c, device=DEV), host[name], name)
    assert all(len(inputs[f"{n}-gon"]["vertices"]) == n for n in BORDERS) and inputs["one long edge next to 500 short ones"]["size"] == (300, 517)
    assert int(host["comb of 2049 spans"].covered.sum()) == 2 * 2049 and int(host["one long edge next to 500 short ones"].covered[0]) > 30000


def test_device_tensors_two_runs_and_both_paint_forms(inputs, host):
    from ullsam_amd.utils import raster as RA
    for name, c in inputs.items():
        args = (T(c["vertices"]), T(c["start"]), T(c["ring_label"]), c["size"], c["order"], c["num"])
        a, b = RA.rasterize_polygons(*args, paint="waves"), RA.rasterize_polygons(*args, paint="waves")
        p = RA.rasterize_polygons(*args, paint="pixels")
        _same(a, host[name], (name, "waves"))
        _same(p, host[name], (name, "pixels"))
        assert all(torch.equal(x, y) for x, y in zip(a, b)), (name, "two runs differ")
    assert RA.PAINT in ("waves", "pixels")
    c = inputs["absent ids"]
    assert torch.equal(run(c, device="cpu").labels, host["absent ids"].labels) and run(c, device=DEV).covered.numel() == 7


def _chain(ops, q, start, label, h, w, k, rank, form, shift=None):
    """every wrapper in turn -> (row0, cnt, nxt, elab, off, keys before the sort, covered, length, raw, labels, area, box, flags)"""
    s = (lambda t: _shifted(t, shift)) if shift else (lambda t: t)
    flags = torch.zeros((ops.RASTER_FLAGS,), dtype=torch.int32, device=DEV)
    row0, cnt, nxt, elab, off, _ = ops.raster_edges(s(q), s(start), s(label), h, w, k, flags)
    crossings = int(flags.cpu()[1])
    keys, _ = ops.raster_keys(s(q), s(row0), s(cnt), s(nxt), s(elab), s(off), crossings, h, w, k, flags)
    srt = torch.sort(keys).values
    covered, length, _ = ops.raster_covered(srt, h, w, k, flags)
    raw, _ = ops.raster_paint(srt, s(rank), h, w, form, s(length), flags)
    label_of = torch.zeros((k + 1,), dtype=torch.int32, device=DEV)
    label_of[(rank + 1).long()] = torch.arange(1, k + 1, dtype=torch.int32, device=DEV)
    labels, area, box, _ = ops.raster_finish(s(raw), s(label_of), flags)
    return row0, cnt, nxt, elab, off, keys, covered, length, raw, labels, area, box, flags


def _fixed(c):
    return T(np.array(R.snap(c["vertices"]), np.int32).reshape(-1, 2)), T(c["start"]), T(c["ring_label"])


def test_raw_kernel_outputs_against_the_loops(small):
    """Every ops wrapper called directly: row ranges and counts, the scan, the keys before the sort, covered, the painted raw frame in both forms, the
    finish."""
    from ullsam_amd import ops
    for name, c in small.items():
        (h, w), start, ring_label = c["size"], c["start"], c["ring_label"]
        want = R.rasterize(c["vertices"], start, ring_label, c["size"], c["order"], c["num"])
        k = len(want.covered)
        qs = R.snap(c["vertices"])
        row0_w, cnt_w = R.edge_rows(qs, start, h)
        edges = R.ring_edges(start)
        q, st, rl = _fixed(c)
        rank = T(want.rank.astype(np.int32))
        for form in ("waves", "pixels"):
            row0, cnt, nxt, elab, off, keys, covered, length, raw, labels, area, box, flags = _chain(ops, q, st, rl, h, w, k, rank, form)
            assert all(t.dtype == torch.int32 for t in (row0, cnt, nxt, elab, off, covered, length, raw, labels, area, box)) and keys.dtype == torch.int64, name
            assert N(row0).tolist() == row0_w and N(cnt).tolist() == cnt_w and N(nxt).tolist() == [j for _, _, j in edges], name
            assert N(elab).tolist() == [int(ring_label[r]) for r, _, _ in edges] and np.array_equal(N(off), np.cumsum(cnt_w) - np.array(cnt_w, np.int64).reshape(-1)), name
            assert flags.cpu().tolist() == [0, sum(cnt_w), 0, 0] and np.array_equal(N(keys), want.keys), name
            assert np.array_equal(N(covered), want.covered) and int(length.sum()) == int(want.covered.sum()) and length.numel() == len(want.keys) // 2, name
            assert tuple(raw.shape) == (h, w) and np.array_equal(N(raw), want.raw), (name, form)
            assert np.array_equal(N(labels), want.labels) and np.array_equal(N(area), want.area) and np.array_equal(N(box).reshape(-1, 4), want.box), (name, form)


def test_unaligned_base_pointers(inputs, host):
    """Every int32 table at a base pointer that is no multiple of 16 bytes (the vertices at no multiple of 8)."""
    from ullsam_amd import ops
    for name in ("cut rectangle", "overlaps, by area", "whole rows of width 65", "2049-gon", "comb of 2049 spans"):
        c = inputs[name]
        h, w = c["size"]
        want = host[name]
        k = want.covered.numel()
        q, st, rl = _fixed(c)
        rank = torch.arange(k, dtype=torch.int32, device=DEV)
        if c["order"] == "area":
            rank[torch.sort(-want.covered.to(DEV).long(), stable=True).indices] = torch.arange(k, dtype=torch.int32, device=DEV)
        for shift, form in ((1, "waves"), (3, "pixels")):
            got = _chain(ops, q, st, rl, h, w, k, rank, form, shift)
            assert got[-1].cpu().tolist()[0] == 0, (name, shift)
            for g, wt in zip((got[9], got[6], got[10], got[11]), want):
                assert torch.equal(g.cpu(), wt), (name, shift)


def test_scan_over_several_workgroups():
    """The three-launch scan where a workgroup's chunk ends, and where its total leaves 31 bits."""
    from ullsam_amd import ops
    rng = np.random.default_rng(11)
    for n in (1, 63) + BORDERS + (3 * 2048, 300 * 2048 + 5):
        v = rng.integers(0, 32768 if n < 60000 else 4, n).astype(np.int32)
        v[rng.integers(0, n)] = 32767
        off, total, flags = ops.raster_scan(T(v))
        assert off.dtype == torch.int32 and np.array_equal(N(off), np.cumsum(v.astype(np.int64)) - v) and int(total.cpu()) == int(v.sum()), n
        assert flags.cpu().tolist() == [0, 0, 0, 0], n
    off, total, flags = ops.raster_scan(torch.full((70000,), 32767, dtype=torch.int32, device=DEV))    # 2.29e9: the total is held, the status says so
    assert int(total.cpu()) == 2 ** 31 - 1 and flags.cpu().tolist() == [4, 0, 0, 0] and int(off[65536].cpu()) == 65536 * 32767 and int(off[-1].cpu()) == 2 ** 31 - 1
    off, total, flags = ops.raster_scan(T(np.array([5, -1, 7, 40000, 2], np.int32)))                  # a value outside 0..32767 counts as 0
    assert N(off).tolist() == [0, 5, 5, 12, 12] and int(total.cpu()) == 14 and flags.cpu().tolist() == [8, 0, 0, 0]
    off0, total, _ = ops.raster_scan(torch.zeros((0,), dtype=torch.int32, device=DEV))
    assert off0.numel() == 0 and int(total.cpu()) == 0


def test_bad_input_raises_and_the_next_call_works(inputs, host):
    from ullsam_amd import ops
    from ullsam_amd.utils import raster as RA
    c = inputs["absent ids"]                              # ids 2 and 5, num = 7
    v, s, l, size = c["vertices"], c["start"], c["ring_label"], c["size"]
    err = ops._lib.UllsamError
    for bad in (dict(ring_label=T(np.array([2, 8], np.int32))), dict(ring_label=[0, 5]), dict(num=4), dict(vertices=np.where(v == v.max(), 65535.6, v)),
                dict(vertices=np.where(v == v.max(), -1e30, v))):
        kw = dict(vertices=v, start=s, ring_label=l, size=size, num=7, device=DEV)
        kw.update(bad)
        with pytest.raises(err):
            RA.rasterize_polygons(**kw)
    q = torch.tensor([[1, 1], [70000, 1], [70000, 5], [1, 5]], dtype=torch.int32, device=DEV)           # integer pixels on the device: times 256 there
    with pytest.raises(err):
        RA.rasterize_polygons(q, [0, 4], [1], (8, 8))
    with pytest.raises(err):
        RA.rasterize_polygons(q.long() * 40000, [0, 4], [1], (8, 8))                                  # beyond 32 bits once multiplied: held, then refused
    q, st, _ = _fixed(c)
    row0, cnt, nxt, elab, off, flags = ops.raster_edges(q, st, T(np.array([2, 8], np.int32)), size[0], size[1], 7)   # the ring is skipped: the other is what it was
    good = ops.raster_edges(q, st, T(l), size[0], size[1], 7)
    assert flags.cpu().tolist()[0] == 1 and N(cnt)[:4].tolist() == N(good[1])[:4].tolist() and N(cnt)[4:].tolist() == [0] * 4 and N(elab).tolist() == [2] * 4 + [0] * 4
    assert int(flags.cpu()[1]) == int(N(good[1])[:4].sum())
    far = q.clone()
    far[5, 0] = 65535 * 256 + 1
    assert ops.raster_edges(far, st, T(l), size[0], size[1], 7)[5].cpu().tolist()[0] == 2
    _same(run(c, device=DEV), host["absent ids"], "the next call")
    zig = np.stack([np.arange(65540) * (3.0 / 65540), np.where(np.arange(65540) % 2 == 0, -1.0, 32768.0)], 1)    # 65540 edges over 32767 rows each
    for dev in (DEV, "cpu"):
        with pytest.raises(err):
            RA.rasterize_polygons(zig, [0, 65540], [1], (32767, 4), device=dev)
    for bad in (dict(start=T(np.array([0, 2, 8], np.int32))), dict(start=T(np.array([0, 4, 9], np.int32))), dict(start=T(np.array([1, 4, 8], np.int32))),
                dict(start=[0, 5, 4, 8]), dict(order="record"), dict(size=(0, 3)), dict(paint="lanes"), dict(vertices=T(np.where(v == v.max(), np.nan, v)))):
        kw = dict(vertices=v, start=s, ring_label=l, size=size, num=7, device=DEV)
        kw.update(bad)
        with pytest.raises(ValueError):
            RA.rasterize_polygons(**kw)
    _same(run(c, device=DEV), host["absent ids"], "after the refusals")


def test_no_rings(inputs, host):
    from ullsam_amd import ops
    for name, k in (("no rings", 0), ("no rings, num = 3", 3)):
        c = inputs[name]
        got = run(c, device=DEV)
        _same(got, host[name], name)
        assert [tuple(t.shape) for t in got] == [tuple(c["size"]), (k,), (k,), (k, 4)] and not got.labels.any()
    empty = torch.zeros((0,), dtype=torch.int32, device=DEV)
    row0, cnt, nxt, elab, off, flags = ops.raster_edges(empty.view(0, 2), torch.zeros((1,), dtype=torch.int32, device=DEV), empty, 4, 7, 3)   # nothing is launched
    keys, _ = ops.raster_keys(empty.view(0, 2), row0, cnt, nxt, elab, off, 0, 4, 7, 3, flags)
    covered, length, _ = ops.raster_covered(keys, 4, 7, 3, flags)
    assert keys.numel() == 0 and keys.dtype == torch.int64 and covered.cpu().tolist() == [0, 0, 0] and length.numel() == 0
    for form in ("waves", "pixels"):
        raw, _ = ops.raster_paint(keys, torch.arange(3, dtype=torch.int32, device=DEV), 4, 7, form, length, flags)
        assert tuple(raw.shape) == (4, 7) and not raw.any()
    assert flags.cpu().tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("conn", (8, 4))
def test_outlines_and_back_on_the_device(conn):
    """label_outlines on the device -> rasterize_polygons on its device tensors returns the label image."""
    from ullsam_amd.utils import outline as O
    from ullsam_amd.utils import raster as RA
    from ullsam_amd.utils import synthetic as S
    for h, w, n, rr in ((300, 517, 90, (6.0, 22.0)), (120, 157, 30, (6.0, 14.0))):
        lab = T(S.label_frame(7, h, w, n, rr))
        out = O.label_outlines(lab, conn)
        assert out.vertices.is_cuda and out.start.is_cuda and out.label.is_cuda
        for form in ("waves", "pixels"):
            back = RA.rasterize_polygons(out.vertices, out.start, out.label, (h, w), num=int(out.loops_of.numel()), paint=form)
            assert back.labels.is_cuda and torch.equal(back.labels, lab) and torch.equal(back.area, back.covered), (h, w, conn, form)
            assert torch.equal(back.covered.long(), torch.bincount(lab.reshape(-1).long(), minlength=out.loops_of.numel() + 1)[1:]), (h, w, conn)


def test_the_chain_composes_on_device_tensors():
    from ullsam_amd.utils import outline as O
    from ullsam_amd.utils import prompts as P
    from ullsam_amd.utils import raster as RA
    from ullsam_amd.utils import synthetic as S
    lab = S.label_frame(7, 120, 157, 30, (6.0, 14.0))
    text = json.dumps(O.to_geojson(O.label_outlines(lab), 0.325, (1234.5, -77.25)))
    got = RA.labels_from_geojson(json.loads(text), lab.shape, 0.325, (1234.5, -77.25), device=DEV)
    assert got.labels.is_cuda and torch.equal(got.labels.cpu(), torch.from_numpy(lab))
    a, b = P.prompts_from_labels(got.labels, seed=3), P.prompts_from_labels(T(lab), seed=3)
    for name, x, y in zip(a._fields, a, b):
        assert (x is None and y is None) or (x.is_cuda and torch.equal(x, y)), name
