"""Splitting the touching objects of a label volume on the GPU (csrc/split3d.hip and split.hip's flat entry points): the device route of
utils.split3d against the host form (itself checked against the plain loops of tests/split3d_ref.py without a GPU), the kernels' raw outputs
through ops against those loops, the status word.  Integer work: every assertion is equality."""
import numpy as np
import pytest
import torch

from tests import distance3d_ref as R3
from tests import distance_ref as R
from tests import split3d_ref as SR3

pytestmark = pytest.mark.gpu
DEV = "cuda"
INF = 2 ** 31 - 1
DEPTHS = (0, 1, 2, 5, 32767)
TILE = (4, 4, 64)                                             # (tz, ty, tx) of the ascent: split3d.hip S3_TZ, S3_TY, S3_TX


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def N(t):
    return t.cpu().numpy().astype(np.int64)


def _same(got, want, what):
    for name, g, w in zip(got._fields, got, want):
        assert g.is_cuda and g.dtype == torch.int32 and tuple(g.shape) == tuple(w.shape) and torch.equal(g.cpu(), w), (what, name)


def _cpu_runs():
    """[(name, volume, spacing, edge)]: the runs of tests/test_split3d_cpu.py."""
    out = [(name, vol, sp, e) for name, vol in R3.cases() for sp in R3.SPACINGS for e in R3.EDGES]
    out += [(name, vol, sp, e) for name, vol in SR3.dense() for sp in SR3.DENSE_SPACINGS for e in R3.EDGES]
    return out + [(name, vol, sp, e) for name, (vol, sp, edges) in SR3.shapes().items() for e in edges]


def _two_ellipsoids():
    """[10, 11, 150]: one object over three tiles in every axis, a long waist between its halves."""
    return (SR3.ball((10, 11, 150), (5, 5, 40), 38, (8, 8, 1)) | SR3.ball((10, 11, 150), (4, 6, 110), 36, (7, 7, 1))).astype(np.int32)


@pytest.fixture(scope="module")
def tiles():
    """[(name, volume)]: volumes chosen to break tiles -- sides of tile - 1, tile, tile + 1 in each axis in turn and together, one object over
    several tiles in each axis, rows that are one run each, a voxel count that is no multiple of 4, and the two contention volumes."""
    from tests import test_distance3d_gpu as TD3
    tz, ty, tx = TILE
    sides = [(tz + a, ty, tx) for a in (-1, 1)] + [(tz, ty + a, tx) for a in (-1, 1)] + [(tz, ty, tx + a) for a in (-1, 1)]
    sides += [(tz + a, ty + a, tx + a) for a in (-1, 0, 1)] + [(2 * tz + 1, 2 * ty - 1, 2 * tx + 1)]
    out = [(f"dense blobs {z} x {h} x {w}", R3.blobs(50 + i, z, h, w, n=8, ids=3)) for i, (z, h, w) in enumerate(sides)]
    out += [(f"whole rows, width {w}", TD3._whole_row_planes(w)) for w in (63, 64, 65, 130)]
    odd = R3.blobs(21, 7, 9, 13, n=9)
    assert odd.size % 4 != 0
    one = SR3.ball((30, 30, 30), (15, 15, 15), 14).astype(np.int32)
    two = (SR3.ball((30, 30, 52), (15, 15, 15), 14) | SR3.ball((30, 30, 52), (15, 15, 36), 14)).astype(np.int32)
    assert int(one.sum()) > 10000 and int(two.sum()) > 20000
    return out + [("one object over several tiles in each axis", _two_ellipsoids()), ("Z * H * W no multiple of 4", odd),
                  ("one ball of thousands of voxels", one), ("two large balls", two)]


@pytest.fixture(scope="module")
def host(tiles):
    """{(name, spacing, edge key, h): the host form's SplitLabels3d}: computed once, shared, never changed."""
    from ullsam_amd.utils import split3d as S3
    out = {(name, sp, R3.edges(e), h): S3.split_labels3d(vol, h, sp, e) for name, vol, sp, e in _cpu_runs() for h in DEPTHS}
    out.update({(name, sp, R3.edges(e), h): S3.split_labels3d(vol, h, sp, e)
                for name, vol in tiles for sp, e in (((1, 1, 1), False), ((5, 2, 2), True)) for h in (0, 1, 5)})
    return out


@pytest.mark.parametrize("spacing", R3.SPACINGS + [None])
def test_device_route_equals_the_host_form_on_the_cpu_cases(host, spacing):
    """spacing None: the dense and the hand-made volumes, each under its own spacings."""
    from ullsam_amd.utils import split3d as S3
    named = dict(R3.cases())
    for name, vol, sp, e in _cpu_runs():
        if (sp == spacing) if name in named else (spacing is None):
            d = T(vol)
            for h in DEPTHS:
                _same(S3.split_labels3d(d, h, sp, e), host[(name, sp, R3.edges(e), h)], (name, sp, e, h))


def test_device_route_on_volumes_that_break_tiles_every_route_two_runs(tiles, host):
    from ullsam_amd.utils import split3d as S3
    for name, vol in tiles:
        d = T(vol)
        for sp, e in (((1, 1, 1), False), ((5, 2, 2), True)):
            for h in (0, 1, 5):
                _same(S3.split_labels3d(d, h, sp, e), host[(name, sp, (bool(e),) * 3, h)], (name, sp, h))
            for route in ("lds", "global"):
                _same(S3.split_labels3d(d, 1, sp, e, route=route), host[(name, sp, (bool(e),) * 3, 1)], (name, sp, route))
        a, b = S3.split_labels3d(d, 1, (5, 2, 2), True), S3.split_labels3d(d, 1, (5, 2, 2), True)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), (name, "two runs differ")
        _same(S3.split_labels3d(vol, 5, device=DEV), host[(name, (1, 1, 1), (False,) * 3, 5)], (name, "numpy volume, device="))
    assert len(host[("one object over several tiles in each axis", (1, 1, 1), (False,) * 3, 0)].parent) == 2     # cut at its waist, tiles from either peak


def test_unaligned_base_pointer(tiles, host):
    from ullsam_amd.utils import split3d as S3
    for name in ("Z * H * W no multiple of 4", "whole rows, width 65", "whole rows, width 64", "dense blobs 5 x 5 x 65", "one object over several tiles in each axis"):
        vol = dict(tiles)[name]
        for off in (1, 3):
            flat = torch.zeros((vol.size + 8,), dtype=torch.int32, device=DEV)
            flat[off:off + vol.size] = T(vol).reshape(-1)
            d = flat[off:off + vol.size].view(vol.shape)
            assert d.is_contiguous() and d.data_ptr() % 16 != 0
            for route in ("lds", "global"):
                _same(S3.split_labels3d(d, 1, route=route), host[(name, (1, 1, 1), (False,) * 3, 1)], (name, off, route))


def test_a_linked_stack_goes_straight_in():
    """utils.synthetic.label_stack 6 x 150 x 260, linked on the device with mode="all" so that cells stacked along z are fused."""
    from ullsam_amd.utils import split3d as S3
    from ullsam_amd.utils import synthetic as S
    from ullsam_amd.utils.stack import link_label_stack
    planes, counts = S.label_stack(5, 6, 150, 260, 60, (6, 22), dz=2.5)
    volume = link_label_stack(planes, counts, mode="all", device=DEV)[0]
    assert volume.is_cuda and volume.dtype == torch.int32 and tuple(volume.shape) == (6, 150, 260)
    vol = volume.cpu().numpy()
    k = int(vol.max())
    for h, e in ((0, False), (2, False), (5, (True, False, False))):
        st, want_st = {}, {}
        want = S3.split_labels3d(vol, h, (5, 2, 2), e, stats=want_st)
        _same(S3.split_labels3d(volume, h, (5, 2, 2), e, num=k, stats=st), want, ("stack", h))
        assert st == want_st and st["parts"] > len(set(vol[vol > 0].tolist())) and st["rounds"] >= 1, (h, st)      # fused objects exist, and are cut
        for route in ("lds", "global"):
            _same(S3.split_labels3d(volume, h, (5, 2, 2), e, route=route), want, ("stack", h, route))


def test_contention_on_one_root_and_one_slot(tiles, host):
    from ullsam_amd.utils import split3d as S3
    for name, parts, pairs in (("one ball of thousands of voxels", 1, 0), ("two large balls", 2, 1)):
        d = T(dict(tiles)[name])
        for _ in range(3):
            st = {}
            got = S3.split_labels3d(d, 1, stats=st)
            _same(got, host[(name, (1, 1, 1), (False,) * 3, 1)], name)
            assert got.parent.numel() == parts == st["basins"] and st["pairs"] == pairs


def _table(keys, vals):
    k, v = N(keys), N(vals)
    return {(int(a), int(b), int(s)) for a, b, s in zip(k[k != 0] >> 32, k[k != 0] & 0xFFFFFFFF, v[k != 0])}


def test_raw_kernel_outputs_against_the_loops():
    """Every wrapper of the route called directly on the hand-made and the dense volumes: the ascent in both routes, flatten, the pass table, rounds
    until rest, collect, relabel."""
    from ullsam_amd import ops
    runs = [(name, vol, sp, e) for name, (vol, sp, edges) in SR3.shapes().items() for e in edges]
    runs += [(name, vol, (2, 3, 5), True) for name, vol in SR3.dense()]
    for name, vol, sp, e in runs:
        z, h, w = vol.shape
        n, k = vol.size, int(vol.max())
        d = T(vol)
        d2 = R3.inner_distance(vol, sp, e)
        dd = T(d2.astype(np.int32))
        want_up = SR3.ascent(vol, d2)
        up, flags = ops.split3d_ascent(d, dd, k, "lds")
        assert up.dtype == torch.int32 and tuple(up.shape) == (z, h, w) and N(up).reshape(-1).tolist() == want_up, (name, e, "lds")
        up, _ = ops.split3d_ascent(d, dd, k, "global", flags=flags)
        assert N(up).reshape(-1).tolist() == want_up, (name, e, "global")
        rep = SR3.roots(want_up)
        ops.split_flatten(up, flags=flags)
        assert N(up).reshape(-1).tolist() == rep, (name, e, "flatten")
        keys, vals, _ = ops.split3d_passes(d, dd, up, 64, k, flags=flags)
        want_edges = SR3.passes(vol, d2, rep)
        assert _table(keys, vals) == {(a, b, s) for (a, b), s in want_edges.items()}, (name, e, "passes")
        assert flags.cpu().tolist() == [0, 0, len(want_edges), 0, 0, 0, 0, 0], (name, e)
        d2f = [int(v) for v in d2.reshape(-1)]
        for depth in (0, 2):
            u = up.clone()
            best = torch.zeros((n,), dtype=torch.int64, device=DEV)
            cur = list(rep)
            for _ in range(8):
                changed = torch.zeros((1,), dtype=torch.int32, device=DEV)
                ops.split_round(keys, vals, d, dd, u, depth, best, changed, k, flags=flags)
                move = SR3.merge_round(want_edges, d2f, cur, depth)
                nxt = list(cur)
                for x, y in move.items():
                    nxt[x] = y
                assert N(u).reshape(-1).tolist() == nxt and int(changed.cpu()) == int(bool(move)) and int(best.abs().sum()) == 0, (name, e, depth)
                if not move:
                    break
                ops.split_flatten(u, flags=flags)
                cur = SR3.roots(nxt)
                assert N(u).reshape(-1).tolist() == cur, (name, e, depth)
            want = SR3.split(vol, depth, sp, e, d2=d2, start=(rep, want_edges))
            parts = int(ops.split_collect(d, u, None, k)[4].cpu())
            assert parts == len(want[1]), (name, e, depth)
            lst, _ = ops.split_collect(d, u, parts, k)
            assert sorted(N(lst).tolist()) == sorted((int(l) << 32) | ((c * h + b) * w + a) for l, (a, b, c) in zip(want[1], want[3])), (name, e, depth)
            got = ops.split3d_relabel(torch.sort(lst).values, d, dd, u, k)
            for g, w_ in zip(got[:5], want[:5]):
                assert g.dtype == torch.int32 and tuple(g.shape) == tuple(w_.shape) and np.array_equal(N(g), w_), (name, e, depth)
            assert got[5].cpu().tolist() == [0] * 8


@pytest.mark.parametrize("edge", [False, True])
def test_one_plane_equals_split_labels_on_the_device(edge):
    from ullsam_amd.utils import split as S
    from ullsam_amd.utils import split3d as S3
    for name, lab in R.cases():
        d = T(lab)
        for h in (0, 1, 32767):
            want = S.split_labels(d, h, edge=edge)
            got = S3.split_labels3d(d[None], h, edge=(False, edge, edge))
            assert got.labels.is_cuda and torch.equal(got.labels[0], want.labels) and torch.equal(got.parent, want.parent), (name, h)
            assert torch.equal(got.peak_r2, want.peak_r2) and torch.equal(got.peak_xyz[:, :2], want.peak_xy) and int(got.peak_xyz[:, 2].abs().sum()) == 0, (name, h)
            assert torch.equal(got.parts_of, want.parts_of), (name, h)


def test_too_many_pairs_or_rounds_raise_and_the_next_call_works():
    from ullsam_amd import ops
    from ullsam_amd.utils import split3d as S3
    name, vol = SR3.dense()[0]
    sp = (2, 3, 5)
    d = T(vol)
    st, want_st = {}, {}
    want = S3.split_labels3d(vol, 1, sp, stats=want_st)
    _same(S3.split_labels3d(d, 1, sp, stats=st), want, name)
    assert st == want_st and st["pairs"] >= 4 and st["rounds"] >= 2
    with pytest.raises(ops._lib.UllsamError, match=f"max_pairs = {st['pairs'] - 1}"):
        S3.split_labels3d(d, 1, sp, max_pairs=st["pairs"] - 1)
    _same(S3.split_labels3d(d, 1, sp, max_pairs=st["pairs"]), want, "the next call")
    with pytest.raises(ops._lib.UllsamError, match=f"max_rounds = {st['rounds']}"):
        S3.split_labels3d(d, 1, sp, max_rounds=st["rounds"])
    _same(S3.split_labels3d(d, 1, sp, max_rounds=st["rounds"] + 1), want, "the next call")


def test_a_bad_label_raises_and_the_next_call_works():
    from ullsam_amd import ops
    from ullsam_amd.utils import split3d as S3
    vol = dict(R3.named_cases())["absent ids"]               # ids 2 and 5
    want = S3.split_labels3d(vol, 1)
    neg = vol.copy()
    neg[0, 0, 0] = -3
    neg[4, 5, 6] = -1                                        # inside id 5
    with pytest.raises(ops._lib.UllsamError):
        S3.split_labels3d(T(neg), 1)
    with pytest.raises(ops._lib.UllsamError):
        S3.split_labels3d(T(vol), 1, num=4)
    d2 = R3.inner_distance(vol)
    for route in ("lds", "global"):
        up, flags = ops.split3d_ascent(T(vol), T(d2.astype(np.int32)), 4, route)       # the id is skipped: the others are what they would be without it
        assert flags.cpu().tolist()[0] == 1 and N(up).reshape(-1).tolist() == SR3.ascent(np.where(vol == 5, 0, vol), d2), route
        bad = np.where(vol == 5, -7, vol)
        up, flags = ops.split3d_ascent(T(bad), T(d2.astype(np.int32)), 5, route)
        assert flags.cpu().tolist()[0] == 1 and N(up).reshape(-1).tolist() == SR3.ascent(np.where(vol == 5, 0, vol), d2), route
    _same(S3.split_labels3d(T(vol), 1), want, "the next call")
    for bad in (lambda: S3.split_labels3d(T(vol), -1), lambda: S3.split_labels3d(T(vol), 1.5), lambda: S3.split_labels3d(T(vol), 1, max_pairs=0),
                lambda: S3.split_labels3d(T(vol), 1, route="fast"), lambda: S3.split_labels3d(T(vol)[0], 1), lambda: S3.split_labels3d(T(vol), 1, (1, 1, 0))):
        with pytest.raises(ValueError):
            bad()


class _Stub:
    shape = (2, 32767, 16384)                                 # 32767^2 + 32767 voxels; nothing but a shape


def test_a_volume_beyond_the_bound_raises_before_anything_is_allocated():
    from ullsam_amd.utils import split3d as S3
    before = torch.cuda.memory_allocated()
    with pytest.raises(ValueError, match="1073709056.*1073676289"):
        S3.split_labels3d(_Stub(), 1, device=DEV)
    assert torch.cuda.memory_allocated() == before
