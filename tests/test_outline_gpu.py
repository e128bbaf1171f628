"""Outlines of label images on the GPU (csrc/outline.hip): the device route of utils.outline against the host form (itself checked against the plain
loops of tests/outline_ref.py without a GPU), the kernels' raw outputs through ops against those loops, the status word, the chain from split_labels.
Integer work: every assertion is equality."""
import numpy as np
import pytest
import torch

from tests import distance_ref as DR
from tests import outline_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
CONN = (8, 4)
DTYPES = (torch.int32, torch.int32, torch.int32, torch.int64, torch.int32, torch.int32, torch.int32)


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def N(t):
    return t.cpu().numpy().astype(np.int64)


def _same(got, want, what):
    for name, g, w, dt in zip(got._fields, got, want, DTYPES):
        assert g.is_cuda and g.dtype == dt and tuple(g.shape) == tuple(w.shape) and torch.equal(g.cpu(), w), (what, name)


@pytest.fixture(scope="module")
def small():
    return list(R.shapes().items())


@pytest.fixture(scope="module")
def shapes(small):
    from tests import test_distance_gpu as TD
    from ullsam_amd.utils import synthetic as S
    return list(small) + DR.cases() + [(f"whole rows, width {w}", TD._whole_rows(w)) for w in (63, 64, 65, 130)] + [
        ("one label over several row tiles", TD._wide()), ("label_frame 120 x 157", S.label_frame(7, 120, 157, 30, (6.0, 14.0))),
        ("label_frame 300 x 517", S.label_frame(7, 300, 517, 90, (6.0, 22.0)))]


@pytest.fixture(scope="module")
def host(shapes):
    """{(name, connectivity): the host form's Outlines}: computed once, shared, never changed."""
    from ullsam_amd.utils import outline as O
    return {(name, c): O.label_outlines(lab, c) for name, lab in shapes for c in CONN}


@pytest.mark.parametrize("c", CONN)
def test_device_route_equals_the_host_form(shapes, host, c):
    from ullsam_amd.utils import outline as O
    for name, lab in shapes:
        _same(O.label_outlines(T(lab), c), host[(name, c)], (name, c))
    big = host[("label_frame 300 x 517", c)]
    assert big.label.numel() > 40 and int(host[("spiral 64 x 64", c)].edges[0]) > 2048 and int((host[("checkerboard 33 x 31", 8)].area2 < 0).sum()) > 400


def test_numpy_labels_with_device_num_and_two_runs(shapes, host):
    from ullsam_amd.utils import outline as O
    for name, lab in shapes:
        _same(O.label_outlines(lab, device=DEV), host[(name, 8)], (name, "numpy labels, device="))
        d = T(lab)
        a, b = O.label_outlines(d, 4), O.label_outlines(d, 4)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), (name, "two runs differ")
    lab = dict(shapes)["absent ids"]
    assert O.label_outlines(T(lab), num=7).loops_of.cpu().tolist() == [0, 1, 0, 0, 1, 0, 0]
    assert torch.equal(O.label_outlines(T(lab), device="cpu").vertices, host[("absent ids", 8)].vertices)


def test_unaligned_base_pointer(shapes, host):
    from ullsam_amd.utils import outline as O
    for name in ("H * W no multiple of 4", "whole rows, width 65", "one label over several row tiles", "checkerboard 33 x 31"):
        lab = dict(shapes)[name]
        h, w = lab.shape
        for off in (1, 3):
            flat = torch.zeros((h * w + 8,), dtype=torch.int32, device=DEV)
            flat[off:off + h * w] = T(lab).reshape(-1)
            d = flat[off:off + h * w].view(h, w)
            assert d.is_contiguous() and d.data_ptr() % 16 != 0
            _same(O.label_outlines(d), host[(name, 8)], (name, off))


def test_raw_kernel_outputs_against_the_loops(small):
    """Every ops wrapper called directly: side masks and offsets, successors, leader and rank, then the loop tables, the ordered compaction, parents."""
    from ullsam_amd import ops
    for name, lab in small:
        h, w = lab.shape
        d = T(lab)
        want_mask = R.side_masks(lab)
        ids = sorted(R.edges(lab))
        at = {e: i for i, e in enumerate(ids)}
        mask, off, flags = ops.outline_sides(d, int(lab.max()))
        assert mask.dtype == torch.uint8 and tuple(mask.shape) == (h, w) and np.array_equal(N(mask), want_mask), name
        cnt = np.array([bin(int(m)).count("1") for m in want_mask.reshape(-1)], np.int64)
        assert off.dtype == torch.int32 and np.array_equal(N(off), np.cumsum(cnt) - cnt), name
        assert flags.cpu().tolist() == [0, len(ids), 0, 0, 0, 0, 0, 0], name
        for c in CONN:
            fl = torch.zeros((ops.OUTLINE_FLAGS,), dtype=torch.int32, device=DEV)
            eid, succ, pdir, _ = ops.outline_successors(d, mask, off, len(ids), c, fl)
            want_succ = R.successors(lab, c)
            assert N(eid).tolist() == ids and N(succ).tolist() == [at[want_succ[e]] for e in ids], (name, c)
            pred = {v: k for k, v in want_succ.items()}
            assert N(pdir).tolist() == [pred[e] % 4 for e in ids], (name, c)
            leader, rank, _ = ops.outline_rank(succ, eid, pdir, fl)
            want_lead, want_rank = R.leader_rank(lab, c)
            assert N(leader).tolist() == [at[want_lead[e]] for e in ids] and N(rank).tolist() == [want_rank[e] for e in ids], (name, c)
            want = R.outlines(lab, c)
            n_loops, n_vert = len(want.label), len(want.vertices)
            lst, _ = ops.outline_collect(d, eid, leader, n_loops + 3, fl)
            assert fl.cpu().tolist() == [0, 0, n_vert, n_loops, n_loops, 0, 0, 0], (name, c)
            keys = torch.sort(lst[:n_loops]).values
            assert N(lst[n_loops:]).tolist() == [0, 0, 0] and N(keys >> 32).tolist() == want.label.tolist(), (name, c)
            lead = (keys & 0xFFFFFFFF).to(torch.int32)
            assert N(lead).tolist() == [at[cyc[0]] for _, cyc in R.cycles(lab, c)], (name, c)
            loop_of = torch.full((len(ids),), -1, dtype=torch.int32, device=DEV)
            loop_of[lead.long()] = torch.arange(n_loops, dtype=torch.int32, device=DEV)
            edges, area2, _ = ops.outline_loops(eid, leader, loop_of, n_loops, w, fl)
            assert edges.dtype == torch.int32 and area2.dtype == torch.int64 and np.array_equal(N(edges), want.edges) and np.array_equal(N(area2), want.area2), (name, c)
            estart = (torch.cumsum(edges, 0) - edges).to(torch.int32)
            reid, corner, _ = ops.outline_order(eid, pdir, leader, rank, loop_of, estart, fl)
            walk = [e for _, cyc in R.cycles(lab, c) for e in cyc]
            assert N(reid).tolist() == walk and N(corner).tolist() == [int(pred[e] % 4 != e % 4) for e in walk], (name, c)
            coff, total = ops.outline_scan(corner)
            assert np.array_equal(N(coff), np.cumsum(N(corner)) - N(corner)) and int(total.cpu()) == n_vert, (name, c)
            vertices = ops.outline_vertices(reid, corner, coff, n_vert, w)
            assert vertices.dtype == torch.int32 and np.array_equal(N(vertices).reshape(-1, 2), want.vertices), (name, c)
            parent, _ = ops.outline_parents(d, mask, off, eid, leader, loop_of, lead, area2, fl)
            assert parent.dtype == torch.int32 and np.array_equal(N(parent), want.parent), (name, c)
            assert fl.cpu().tolist() == [0, 0, n_vert, n_loops, n_loops, 0, 0, 0], (name, c)


def test_scan_over_several_workgroups():
    """The three-launch scan where a workgroup's chunk ends: lengths around 2048 and its multiples, values 0 and non-zero."""
    from ullsam_amd import ops
    rng = np.random.default_rng(11)
    for n in (1, 63, 2047, 2048, 2049, 3 * 2048, 5 * 2048 + 77, 300 * 2048 + 5):
        v = (rng.integers(0, 3, n) * rng.integers(0, 2, n)).astype(np.uint8)
        off, total = ops.outline_scan(T(v))
        nz = (v != 0).astype(np.int64)
        assert np.array_equal(N(off), np.cumsum(nz) - nz) and int(total.cpu()) == int(nz.sum()), n


def test_a_bad_label_raises_and_the_next_call_works(shapes, host):
    from ullsam_amd import ops
    from ullsam_amd.utils import outline as O
    lab = dict(shapes)["absent ids"]                      # ids 2 and 5
    neg = lab.copy()
    neg[0, 0] = -3
    neg[7, 8] = -1                                        # inside id 5
    with pytest.raises(ops._lib.UllsamError):
        O.label_outlines(T(neg))
    with pytest.raises(ops._lib.UllsamError):
        O.label_outlines(T(lab), num=4)
    mask, off, flags = ops.outline_sides(T(lab), 4)       # the id is skipped: the others are what they would be without it
    assert flags.cpu().tolist()[:2] == [1, 14] and np.array_equal(N(mask), R.side_masks(np.where(lab == 5, 0, lab)))
    _same(O.label_outlines(T(lab)), host[("absent ids", 8)], "the next call")
    for bad in (lambda: O.label_outlines(T(lab), connectivity=6), lambda: O.label_outlines(T(lab)[0])):
        with pytest.raises(ValueError):
            bad()


def test_an_empty_frame(shapes, host):
    from ullsam_amd import ops
    from ullsam_amd.utils import outline as O
    d = T(np.zeros((6, 5), np.int32))
    got = O.label_outlines(d)
    _same(got, host[("an empty frame", 8)], "an empty frame")
    assert [tuple(t.shape) for t in got] == [(0,), (1,), (0,), (0,), (0,), (0, 2), (0,)] and got.start.cpu().tolist() == [0]
    mask, off, flags = ops.outline_sides(d, 0)
    eid, succ, pdir, _ = ops.outline_successors(d, mask, off, 0, 8, flags)            # E = 0: nothing is launched
    leader, rank, _ = ops.outline_rank(succ, eid, pdir, flags)
    assert eid.numel() == 0 and leader.numel() == 0 and rank.numel() == 0 and flags.cpu().tolist() == [0] * 8
    off0, total = ops.outline_scan(torch.zeros((0,), dtype=torch.uint8, device=DEV))
    assert off0.numel() == 0 and int(total.cpu()) == 0


def test_the_chain_composes_on_device_tensors(shapes):
    from ullsam_amd.utils import outline as O
    from ullsam_amd.utils import split as SP
    lab = dict(shapes)["label_frame 120 x 157"]
    parts = SP.split_labels(T(lab), 1).labels
    assert parts.is_cuda
    out = O.label_outlines(parts)
    assert out.vertices.is_cuda and np.array_equal(R.fill(out, *lab.shape), N(parts))
    assert int(out.loops_of.numel()) == int(parts.max()) and int((out.loops_of > 0).sum()) == int(parts.max())
