"""Simplified outlines on the GPU (csrc/simplify.hip): the device route of utils.simplify against the numpy form (itself checked against the plain
definition of tests/simplify_ref.py without a GPU), the kernels' raw outputs through ops against that definition, the status word, the chain to
rasterize_polygons.  Integer work: every assertion is equality."""
import numpy as np
import pytest
import torch

from tests import outline_ref as R
from tests import simplify_ref as SR

pytestmark = pytest.mark.gpu
DEV = "cuda"
CONN = (8, 4)
TS = (0, 128, 256, 640)
DTYPES = (torch.int32, torch.int32, torch.int32, torch.int64, torch.int32, torch.int32, torch.int32)


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def N(t):
    return t.cpu().numpy().astype(np.int64)


def _same(got, want, what):
    for name, g, w, dt in zip(got.outlines._fields, got.outlines, want.outlines, DTYPES):
        assert g.is_cuda and g.dtype == dt and tuple(g.shape) == tuple(w.shape) and torch.equal(g.cpu(), w), (what, name)
    assert got.source.is_cuda and got.source.dtype == torch.int32 and torch.equal(got.source.cpu(), want.source), (what, "source")


def noise3():
    """96 x 128, three values: thousands of candidates in loops that wind through the whole frame"""
    return np.random.default_rng(12).integers(0, 3, (96, 128)).astype(np.int32)


@pytest.fixture(scope="module")
def shapes():
    from ullsam_amd.utils import synthetic as S
    out = SR.all_images()
    out["noise 96 x 128, three values"] = noise3()
    out["noise 96 x 128, two values"] = np.random.default_rng(12).integers(0, 2, (96, 128)).astype(np.int32)
    out["label_frame 120 x 157"] = S.label_frame(7, 120, 157, 30, (6.0, 14.0))
    return out


@pytest.fixture(scope="module")
def host(shapes):
    """{(name, connectivity, T): the numpy form's result}: computed once, shared, never changed."""
    from ullsam_amd.utils import simplify as S
    return {(name, c, t): S.simplify_outlines(lab, t / 256, c) for name, lab in shapes.items() for c in CONN for t in TS}


@pytest.mark.parametrize("c", CONN)
def test_device_route_equals_the_numpy_form(shapes, host, c):
    from ullsam_amd.utils import simplify as S
    for name, lab in shapes.items():
        d = T(lab)
        for t in TS:
            _same(S.simplify_outlines(d, t / 256, c), host[(name, c, t)], (name, c, t))
    # many workgroups of candidates, and (connectivity 8) one loop with more candidates than a workgroup has threads
    assert int(host[("spiral 64 x 64", c, 0)].outlines.edges[0]) > 2048 and int(host[("noise 96 x 128, three values", c, 0)].outlines.vertices.shape[0]) > 15000
    big = host[("noise 96 x 128, two values", 8, 0)].outlines
    assert int((big.start[1:] - big.start[:-1]).max()) > 1024


def test_numpy_labels_with_device_and_two_runs(shapes, host):
    from ullsam_amd.utils import simplify as S
    for name, lab in shapes.items():
        _same(S.simplify_outlines(lab, 1.0, device=DEV), host[(name, 8, 256)], (name, "numpy labels, device="))
        d = T(lab)
        a, b = S.simplify_outlines(d, 0.5, 4), S.simplify_outlines(d, 0.5, 4)
        assert all(torch.equal(x, y) for x, y in zip(a.outlines, b.outlines)) and torch.equal(a.source, b.source), (name, "two runs differ")
    lab = shapes["absent ids"]
    assert S.simplify_outlines(T(lab), 0.5, num=7).outlines.loops_of.cpu().tolist() == [0, 1, 0, 0, 1, 0, 0]
    assert torch.equal(S.simplify_outlines(T(lab), 0.5, device="cpu").outlines.vertices, host[("absent ids", 8, 128)].outlines.vertices)


def test_unaligned_base_pointer(shapes, host):
    from ullsam_amd.utils import simplify as S
    for name in ("H * W no multiple of 4", "checkerboard 33 x 31", "a tiling without background 41 x 39"):
        lab = shapes[name]
        h, w = lab.shape
        for off in (1, 3):
            flat = torch.zeros((h * w + 8,), dtype=torch.int32, device=DEV)
            flat[off:off + h * w] = T(lab).reshape(-1)
            d = flat[off:off + h * w].view(h, w)
            assert d.is_contiguous() and d.data_ptr() % 16 != 0
            _same(S.simplify_outlines(d, 1.0), host[(name, 8, 256)], (name, off))


def test_more_rounds_than_one_read_back_block(shapes, host):
    """The host reads the round counters once per block of rounds: runs that need several blocks (the spiral: more rounds than the longest block), and
    blocks of other lengths, give the same."""
    from ullsam_amd.utils import simplify as S
    for name, least in (("spiral 64 x 64", S.ROUND_BLOCK_MAX), ("noise 96 x 128, three values", S.ROUND_BLOCK)):
        d = T(shapes[name])
        got, info = S._run(d, 0.5, 8)
        assert info["rounds"] > least and info == S._run(shapes[name], 0.5, 8)[1]
        _same(got, host[(name, 8, 128)], "the default blocks")
        for block in (1, 3, 64):
            res, inf = S._run(d, 0.5, 8, block=block)
            _same(res, host[(name, 8, 128)], block)
            assert inf == info


def test_a_valid_hole_goes_with_its_parent(shapes):
    """The outer ring of label 1 is three collinear fixed points at 7 px; its hole keeps a valid ring and is dropped by the parent rule alone."""
    from ullsam_amd.utils import simplify as S
    lab = shapes["a valid hole whose parent drops"]
    for c in CONN:
        want = S.simplify_outlines(lab, 7.0, c)
        got = S.simplify_outlines(T(lab), 7.0, c)
        _same(got, want, c)
        assert got.source.cpu().tolist() == [2, 3, 5, 6] and got.outlines.parent.cpu().tolist() == [0, 1, 2, 3]
        ref = SR.simplify(lab, 7 * 256, c)
        assert len(ref.rings[1]) == 3 and ref.src.area2[1] < 0                            # (the hole's own ring: tests/test_simplify_cpu.py holds its area)


def test_one_loop_of_thousands_of_candidates():
    """A comb of 1100 teeth: one loop of 4400 candidates next to small loops.  At a tolerance of one pixel the teeth go in one round."""
    from ullsam_amd.utils import simplify as S
    lab = np.zeros((9, 2203), np.int32)
    lab[2, 1:2202] = 1
    lab[1, 1:2202:2] = 1
    lab[5:8, 3:9] = 2
    lab[5:8, 20:31] = 3
    lab[6, 22:29] = 0
    want, info = S._run(lab, 1.0, 8)
    assert info["candidates"] > 4400 and info["rounds"] == 1 and want.source.tolist() == [0, 1, 2]       # (the thin hole of 3 goes)
    got, inf = S._run(T(lab), 1.0, 8)
    _same(got, want, "the comb")
    assert inf == info


def test_raw_kernel_outputs_against_the_definition(shapes):
    """Every ops wrapper called directly on outline_order's tables: the flags, the candidate tables, the anchors, the segments, one round at a time,
    the rings."""
    from ullsam_amd import ops
    from ullsam_amd.utils import simplify as S
    for name in ("noise 24 x 31", "tied farthest anchors", "loops with one fixed point", "two equal bumps on a shared border", "nested rings 9 x 9"):
        lab = shapes[name]
        h, w = lab.shape
        d = T(lab)
        for c in CONN:
            _, reid, corner, estart, _ = S._ordered_device(d, int(lab.max()), c)
            ref = SR.simplify(lab, 200, c)
            walk = [e for _, cyc in R.cycles(lab, c) for e in cyc]
            ed = R.edges(lab)
            assert N(reid).tolist() == walk
            cand, flags = ops.simplify_flags(d, reid, corner)
            fixed = [SR.is_fixed(lab, *ed[e][1]) for e in walk]
            assert N(cand).tolist() == [3 if f else int(k) for f, k in zip(fixed, N(corner).tolist())], (name, c)
            coff, total = ops.outline_scan(cand)
            pts = [p for cs in ref.cands for p in cs]
            assert int(total.cpu()) == len(pts)
            cxy, cloop, kept, nfixed, _ = ops.simplify_candidates(reid, cand, coff, estart, len(pts), h, w, flags)
            assert N(cxy).tolist() == [y << 16 | x for x, y in pts] and N(cloop).tolist() == [i for i, cs in enumerate(ref.cands) for _ in cs], (name, c)
            assert N(kept).tolist() == [int(SR.is_fixed(lab, *p)) for p in pts] and N(nfixed).tolist() == [sum(SR.is_fixed(lab, *p) for p in cs) for cs in ref.cands]
            cstart = torch.cat([coff[estart.long()], total]).to(torch.int32)
            first = SR.simplify(lab, 255 * 256, c)                   # at the largest tolerance few candidates besides the first kept ones stay
            ops.simplify_anchors(cxy, cloop, nfixed, kept, flags)
            base = N(cstart).tolist()
            want0 = [int(any(SR.is_fixed(lab, *p) for p in cs)) for cs in ref.cands]
            for i, cs in enumerate(ref.cands):
                k = N(kept)[base[i]:base[i + 1]].tolist()
                if want0[i]:
                    assert k == [int(SR.is_fixed(lab, *p)) for p in cs], (name, c, i)
                else:
                    assert [j for j, v in enumerate(k) if v] == first.rings[i] and len(first.rings[i]) == 2, (name, c, i)
            pa, pb, _ = ops.simplify_segments(kept, cloop, cstart, flags)
            kk, lp, pa_h, pb_h = N(kept), N(cloop), N(pa).tolist(), N(pb).tolist()
            for i in range(len(pts)):
                lo, hi = base[lp[i]], base[lp[i] + 1]
                n = hi - lo
                if kk[i]:
                    assert pa_h[i] == -1 and pb_h[i] == -1
                else:
                    back = next(lo + (i - lo - s) % n for s in range(1, n + 1) if kk[lo + (i - lo - s) % n])
                    fwd = next(lo + (i - lo + s) % n for s in range(1, n + 1) if kk[lo + (i - lo + s) % n])
                    assert (pa_h[i], pb_h[i]) == (back, fwd), (name, c, i)
            total_kept, rounds = int(kk.sum()), 0
            while True:
                counts, _ = ops.simplify_rounds(cxy, cloop, cstart, 200, 1, pa, pb, kept, flags)
                got = int(counts.cpu()[0])
                total_kept += got
                assert int(kept.sum()) == total_kept
                if got == 0:
                    break
                rounds += 1
            assert rounds >= 1 and N(kept).tolist() == [int(j in ring) for cs, ring in zip(ref.cands, ref.rings) for j in range(len(cs))], (name, c)
            voff, total = ops.outline_scan(kept)
            vertices, nvert, area2, _ = ops.simplify_rings(cxy, cloop, kept, voff, total, cstart, total_kept, flags)
            assert N(vertices).tolist() == [list(cs[j]) for cs, ring in zip(ref.cands, ref.rings) for j in ring], (name, c)
            assert N(nvert).tolist() == [len(r) for r in ref.rings]
            want_area = [sum(p[0] * q[1] - q[0] * p[1] for p, q in zip(r, r[1:] + r[:1])) for r in ([cs[j] for j in ring] for cs, ring in zip(ref.cands, ref.rings))]
            assert area2.dtype == torch.int64 and N(area2).tolist() == want_area and flags.cpu().tolist() == [0, 0, 0, 0], (name, c)


def test_a_bad_label_raises_and_the_next_call_works(shapes, host):
    from ullsam_amd import ops
    from ullsam_amd.utils import simplify as S
    lab = shapes["absent ids"]                            # ids 2 and 5
    neg = lab.copy()
    neg[0, 0] = -3
    neg[7, 8] = -1
    with pytest.raises(ops._lib.UllsamError):
        S.simplify_outlines(T(neg), 1.0)
    with pytest.raises(ops._lib.UllsamError):
        S.simplify_outlines(T(lab), 1.0, num=4)
    _same(S.simplify_outlines(T(lab), 1.0), host[("absent ids", 8, 256)], "the next call")
    for bad in (lambda: S.simplify_outlines(T(lab), 1.0, connectivity=6), lambda: S.simplify_outlines(T(lab)[0], 1.0), lambda: S.simplify_outlines(T(lab), -1.0),
                lambda: S.simplify_outlines(T(lab), 256.0)):
        with pytest.raises(ValueError):
            bad()
    # a hand-made table: indices outside their range raise the status word and nothing is indexed with them
    d = T(lab)
    _, reid, corner, estart, _ = S._ordered_device(d, 5, 8)
    wild = reid.clone()
    wild[3] = 2 ** 30
    cand, flags = ops.simplify_flags(d, wild, corner)
    assert flags.cpu().tolist()[0] == 1 and int(cand[3]) == 0


def test_an_empty_frame(shapes, host):
    from ullsam_amd.utils import simplify as S
    got = S.simplify_outlines(T(np.zeros((6, 5), np.int32)), 1.0)
    _same(got, host[("an empty frame", 8, 256)], "an empty frame")
    assert [tuple(t.shape) for t in got.outlines] == [(0,), (1,), (0,), (0,), (0,), (0, 2), (0,)] and tuple(got.source.shape) == (0,)


def test_the_chain_composes_on_device_tensors(shapes):
    """At tolerance 0 the rings enclose what label_outlines' rings enclose: rasterising them gives the label image back."""
    from ullsam_amd.utils import raster as RA
    from ullsam_amd.utils import simplify as S
    for name in ("label_frame 120 x 157", "a tiling without background 41 x 39", "noise 24 x 31"):
        lab = shapes[name]
        out = S.simplify_outlines(T(lab), 0).outlines
        assert out.vertices.is_cuda
        back = RA.rasterize_polygons(out.vertices, out.start, out.label, lab.shape, num=int(out.loops_of.numel()))
        assert back.labels.is_cuda and np.array_equal(N(back.labels), lab), name
