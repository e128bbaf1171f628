"""utils.split3d without a GPU: the numpy host form against the plain loops of tests/split3d_ref.py, the one-plane equality with utils.split, the
homogeneity under a common factor, the properties the definition promises, hand-made objects with part counts pinned from the loops, the ABI, the
kernels' resources, argument errors.  Integer work: every assertion is equality."""
import os
import re
import sys

import numpy as np
import pytest
import torch

from tests import distance3d_ref as R3
from tests import distance_ref as R
from tests import split3d_ref as SR3
from ullsam_amd import _lib
from ullsam_amd.utils import split as S
from ullsam_amd.utils import split3d as S3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = 2 ** 31 - 1
DEPTHS = (0, 1, 2, 5, 32767)


def N(t):
    return t.numpy().astype(np.int64)


def _equal(got, want, what):
    assert isinstance(got, S3.SplitLabels3d) and all(t.dtype == torch.int32 for t in got), what
    for name, g, w in zip(got._fields, got, want):
        assert tuple(g.shape) == tuple(w.shape) and np.array_equal(N(g), w), (what, name)


def _runs():
    """[(name, volume, spacing, edge)]: distance3d_ref's cases under every spacing and edge of its lists, denser random volumes whose objects have
    several basins under two spacings and every edge, and the hand-made volumes under theirs."""
    out = [(name, vol, sp, e) for name, vol in R3.cases() for sp in R3.SPACINGS for e in R3.EDGES]
    out += [(name, vol, sp, e) for name, vol in SR3.dense() for sp in SR3.DENSE_SPACINGS for e in R3.EDGES]
    return out + [(name, vol, sp, e) for name, (vol, sp, edges) in SR3.shapes().items() for e in edges]


@pytest.fixture(scope="module")
def reference():
    """{(name, spacing, edge key, h): split3d_ref.split}: computed once, shared, never changed.  The brute-force D2 and the basins of a run do not
    depend on h and are computed once per run."""
    out = {}
    named = dict(R3.cases())
    for name, vol, sp, e in _runs():
        d2 = R3.reference(name, "inner", sp, e) if name in named else R3.inner_distance(vol, sp, e)
        start = SR3.basins(vol, d2)
        for h in DEPTHS:
            out[(name, sp, R3.edges(e), h)] = SR3.split(vol, h, sp, e, d2=d2, start=start)
    return out


def test_the_cases_cover_what_they_should(reference):
    shapes = [vol.shape for name, vol in R3.cases() if name.startswith("blobs")]
    assert (1, 1, 1) in shapes and any(s[0] == 1 and min(s[1:]) > 1 for s in shapes) and any(s[1] == s[2] == 1 and s[0] > 1 for s in shapes)
    rounds = [r[5] for r in reference.values()]
    assert max(rounds) >= 2 and min(rounds) == 0                                  # the merge loop runs more than once somewhere
    assert any(len(r[1]) > len(reference[k[:3] + (32767,)][1]) for k, r in reference.items() if k[3] == 0)          # h matters
    for lo, hi in zip(DEPTHS, DEPTHS[1:]):                                        # every step of the depths takes a part away somewhere
        assert any(len(reference[k[:3] + (lo,)][1]) > len(reference[k[:3] + (hi,)][1]) for k in reference), (lo, hi)
    assert all(100 <= vol.size <= 1600 or name == "a 1 x 1 x n line" for name, (vol, _, _) in SR3.shapes().items())


@pytest.mark.parametrize("spacing", R3.SPACINGS + [None])
def test_host_form_against_the_loops(reference, spacing):
    """spacing None: the hand-made volumes, each under its own spacing."""
    named = dict(R3.cases())
    for name, vol, sp, e in _runs():
        if (sp == spacing) if name in named else (spacing is None):
            for h in DEPTHS:
                _equal(S3.split_labels3d(vol, h, sp, e), reference[(name, sp, R3.edges(e), h)], (name, sp, e, h))


def _parts(vol, h, sp, e=False):
    return int(S3.split_labels3d(vol, h, sp, e).parent.numel())


def test_hand_made_objects(reference):
    """The part counts are the loops'; the host form equals them (above), so they are asserted on the loops' results here."""
    sh = SR3.shapes()
    count = lambda name, e=False: [len(reference[(name, sh[name][1], R3.edges(e), h)][1]) for h in DEPTHS]
    assert count("two balls fused along z, spacing (1, 1, 1): a neck") == [2, 2, 1, 1, 1]
    assert count("two balls fused along z, spacing (1, 3, 3): no neck") == [1, 1, 1, 1, 1]       # the same voxels: the spacing decides
    assert count("two balls fused along x") == [2, 2, 1, 1, 1]
    assert count("a neck diagonal in all three axes") == [2, 1, 1, 1, 1]
    vol = sh["a neck diagonal in all three axes"][0]                                              # one voxel pair holds it together, corner to corner
    assert vol[4, 4, 4] == vol[5, 5, 5] == 1 and vol[4:6, 4:6, 4:6].sum() == 2 and SR3.component_count(vol) == 1
    assert count("one id in two unconnected pieces") == [2, 2, 2, 2, 2] and count("absent ids") == [2, 2, 2, 2, 2]
    assert reference[("absent ids", (2, 3, 5), (False,) * 3, 1)][4].tolist() == [0, 1, 0, 0, 1]
    for e in R3.EDGES:
        assert count("a 1 x 1 x n line", e) == [3, 3, 3, 3, 3]
        assert count("an object touching the border", e)[-1] == 1 and count("Z = 1", e)[0] == count("Z = 2", e)[0] == 2
    name = "a U-shaped plateau"                                                                   # D2 = 4 along the whole centre line: two roots of equal D2
    vol = sh[name][0]
    d2 = R3.inner_distance(vol)
    rep, edges = SR3.basins(vol, d2)
    roots = sorted({r for p, r in enumerate(rep) if vol.reshape(-1)[p] > 0})
    assert len(roots) == 2 and {int(d2.reshape(-1)[r]) for r in roots} == {4} and list(edges.values()) == [4]
    got = S3.split_labels3d(vol, 0)                                                               # P = S: t = 0 at h = 0
    assert got.parent.tolist() == [1] and got.peak_r2.tolist() == [4] and np.array_equal(N(got.labels), vol)
    got = S3.split_labels3d(sh["equal peaks"][0], 2)                                              # peaks 9 and 9: the smaller index keeps its place
    assert got.parent.tolist() == [1] and got.peak_r2.tolist() == [9] and got.peak_xyz.tolist() == [[3, 3, 3]]
    assert S3.split_labels3d(sh["equal peaks"][0], 1).peak_xyz.tolist() == [[3, 3, 3], [11, 3, 3]]


def test_two_fused_balls_at_anisotropic_spacing():
    """Two balls of radius 22 (spacing units) at spacing (5, 2, 2), centres 5 planes apart in 9 x 40 x 40: cut at min_depth <= 2, whole from 3 on.
    The counts are pinned from the loops on the brute-force map."""
    sp = (5, 2, 2)
    vol = (SR3.ball((9, 40, 40), (2, 20, 20), 22, sp) | SR3.ball((9, 40, 40), (7, 20, 20), 22, sp)).astype(np.int32)
    d2 = R3.inner_distance(vol, sp)
    start = SR3.basins(vol, d2)
    want = [SR3.split(vol, h, sp, d2=d2, start=start) for h in range(7)]
    assert [len(w[1]) for w in want] == [2, 2, 2, 1, 1, 1, 1]
    assert want[0][2].tolist() == [488, 488] and want[0][3].tolist() == [[20, 20, 2], [20, 20, 7]]
    for h in range(7):
        _equal(S3.split_labels3d(vol, h, sp), want[h], h)
    assert [_parts(vol, h, sp) for h in (0, 1, 2)] == [2, 2, 2] and [_parts(vol, h, sp) for h in (4, 5, 100, 32767)] == [1, 1, 1, 1]


@pytest.mark.parametrize("edge", [False, True])
def test_one_plane_equals_split_labels(edge):
    for name, lab in R.cases():
        for h in (0, 1, 2, 32767):
            want = S.split_labels(lab, h, edge=edge)
            got = S3.split_labels3d(lab[None], h, edge=(False, edge, edge))
            assert torch.equal(got.labels[0], want.labels) and torch.equal(got.parent, want.parent) and torch.equal(got.peak_r2, want.peak_r2), (name, h)
            assert torch.equal(got.peak_xyz[:, :2], want.peak_xy) and int(got.peak_xyz[:, 2].abs().sum()) == 0, (name, h)
            assert torch.equal(got.parts_of, want.parts_of), (name, h)


def test_homogeneity():
    """Spacing and min_depth times a common factor: the same labels, peak_r2 times the factor squared."""
    for name, vol, sp, e in _runs():
        if sp in ((1, 1, 1), (2, 3, 5), (3, 1, 1), (1, 3, 3)):
            for h in (0, 1, 2, 5):
                base = S3.split_labels3d(vol, h, sp, e)
                for f in (2, 3):
                    got = S3.split_labels3d(vol, f * h, tuple(f * s for s in sp), e)
                    finite = base.peak_r2 < INF                              # (INF: no other voxel at all, at any spacing)
                    assert torch.equal(got.labels, base.labels) and torch.equal(got.parent, base.parent) and torch.equal(got.peak_xyz, base.peak_xyz), (name, h, f)
                    assert torch.equal(got.peak_r2[finite], base.peak_r2[finite] * (f * f)) and bool((got.peak_r2[~finite] == INF).all()), (name, h, f)


def test_properties(reference):
    """Partition, one parent per part, the numbering, every part 26-connected, the peaks, and h = 32767 = the 26-connected components."""
    try:
        import scipy.ndimage as ndi
    except ImportError:
        ndi = None
    full = np.ones((3, 3, 3), int)
    for name, vol, sp, e in _runs():
        if sp not in ((1, 1, 1), (2, 3, 5), (3, 1, 1), (1, 3, 3)):
            continue
        k = int(vol.max())
        components = SR3.component_count(vol)
        if ndi is not None:
            assert components == sum(ndi.label(vol == i, structure=full)[1] for i in range(1, k + 1)), name
        d2 = N(S3.D3.inner_distance3d(vol, sp, e))                                # the ORIGINAL volume's map: a part's peak is the maximum of this D2 over
        for h in DEPTHS:                                                          # the part's voxels, not the map the parts volume would have
            out, parent, r2, xyz, parts_of = (N(t) for t in S3.split_labels3d(vol, h, sp, e))
            kk = len(parent)
            assert np.array_equal(out > 0, vol > 0) and sorted(set(out[out > 0].tolist())) == list(range(1, kk + 1)), (name, h)      # a partition
            assert np.array_equal(np.concatenate([[0], parent])[out], vol), (name, h)                                              # one parent each
            assert np.array_equal(parts_of, np.bincount(parent, minlength=k + 1)[1:k + 1]), (name, h)
            reps = (xyz[:, 2] * vol.shape[1] + xyz[:, 1]) * vol.shape[2] + xyz[:, 0]
            order = list(zip(parent.tolist(), reps.tolist()))
            assert order == sorted(order) and len(set(order)) == kk, (name, h)
            assert SR3.component_count(out) == kk, (name, h)                                                       # every part is 26-connected
            want_r2, want_xyz = R3.object_depth(out, kk, d2)
            assert np.array_equal(r2, want_r2) and np.array_equal(xyz, want_xyz.reshape(-1, 3)), (name, h)
            assert kk >= components and (h < 32767 or kk == components), (name, h)
            # (sqrt(peak_r2) <= 32767 + min(spacing) on these volumes: the sufficient condition of DESIGN.md for h = 32767)
            assert all(p == INF or p <= (32767 + min(sp)) ** 2 for p in r2.tolist()), name


def test_nothing_crosses_a_border_between_labels_and_empty_volumes():
    vol = np.zeros((4, 6, 12), np.int32)
    vol[1:3, 1:5, 1:6] = 1
    vol[1:3, 1:5, 6:11] = 2
    for h in DEPTHS:
        got = S3.split_labels3d(vol, h, (2, 1, 1))
        assert got.parent.tolist() == [1, 2] and got.parts_of.tolist() == [1, 1] and np.array_equal(N(got.labels), vol), h
    got = S3.split_labels3d(np.zeros((3, 4, 5), np.int32), 1)
    assert [tuple(t.shape) for t in got] == [(3, 4, 5), (0,), (0,), (0, 3), (0,)] and int(got.labels.abs().sum()) == 0
    full = np.full((3, 4, 5), 1, np.int32)                                        # all INF: one plateau, joined through P = S
    for h in DEPTHS:
        got = S3.split_labels3d(full, h)
        assert got.parent.tolist() == [1] and got.peak_r2.tolist() == [INF] and got.peak_xyz.tolist() == [[0, 0, 0]]
    assert S3.split_labels3d(full, 0, edge=True).peak_xyz.tolist() == [[1, 1, 1]]       # D2 = min(4, 4, (x + 1)^2, (5 - x)^2): 4 from (1, 1, 1) on
    got = S3.split_labels3d(dict(R3.named_cases())["absent ids"], 1, num=7)
    assert got.parts_of.tolist() == [0, 1, 0, 0, 1, 0, 0] and got.parent.tolist() == [2, 5]


class _Stub:
    def __init__(self, *shape):
        self.shape = shape


def test_errors_state_their_numbers():
    vol = R3.blobs(5, 6, 7, 8)
    bad = vol.copy()
    bad[0, 0, 0] = -1
    for call, text in ((lambda: S3.split_labels3d(vol[0], 1), r"\(7, 8\)"), (lambda: S3.split_labels3d(_Stub(1, 32768, 2), 1), "32768"),
                       (lambda: S3.split_labels3d(_Stub(32767, 32767, 2), 1), str(32767 * 32767 * 2)),
                       (lambda: S3.split_labels3d(_Stub(1, 32767, 32767), 1, (1, 2, 1)), "5368053780"),             # B = 5 * 32766^2; 32767^2 voxels are allowed
                       (lambda: S3.split_labels3d(_Stub(3, 32768, 32767), 1), "32768"),
                       (lambda: S3.split_labels3d(_Stub(2, 32767, 16384), 1), "1073709056.*1073676289"),           # 32767^2 + 32767 voxels: one plane too many
                       (lambda: S3.split_labels3d(vol, 1, (1, 1)), r"\(1, 1\)"), (lambda: S3.split_labels3d(vol, 1, (1, 1, 0)), "46340"),
                       (lambda: S3.split_labels3d(vol, 1, (1, 2.0, 1)), "2.0"), (lambda: S3.split_labels3d(vol, 1, (46340, 46340, 46340)), "2\\^31 - 2"),
                       (lambda: S3.split_labels3d(vol, 1, edge=(True, False)), "triple"),
                       (lambda: S3.split_labels3d(vol, -1), "-1 must lie in 0..32767"), (lambda: S3.split_labels3d(vol, 32768), "32768 must lie in 0..32767"),
                       (lambda: S3.split_labels3d(vol, 1.0), "1.0"), (lambda: S3.split_labels3d(vol, True), "True"),
                       (lambda: S3.split_labels3d(bad, 1), "negative"),
                       (lambda: S3.split_labels3d(vol, 1, max_pairs=0), "max_pairs = 0"), (lambda: S3.split_labels3d(vol, 1, max_pairs=2 ** 30 + 1), str(2 ** 30 + 1)),
                       (lambda: S3.split_labels3d(vol, 1, max_rounds=0), "max_rounds = 0"), (lambda: S3.split_labels3d(vol, 1, route="fast"), "fast"),
                       (lambda: S3.split_labels3d(vol, 1, num=int(vol.max()) - 1), f"0..{int(vol.max()) - 1}"), (lambda: S3.split_labels3d(vol, 1, num=-1), "-1")):
        with pytest.raises(ValueError, match=text):
            call()
    assert S3.MAX_VOXELS == 32767 ** 2 == 1073676289
    for volume in (vol, torch.from_numpy(vol), torch.from_numpy(vol.astype(np.int64))):
        got = S3.split_labels3d(volume, 1, device="cpu")
        assert not got.labels.is_cuda and np.array_equal(N(got.labels), N(S3.split_labels3d(vol, 1).labels))


def test_stats_and_the_limits_on_pairs_and_rounds(reference):
    named = dict(SR3.dense())
    key = max((k for k in reference if k[0] in named), key=lambda k: (reference[k][5], -k[3]))    # the run with the most rounds, at its smallest h
    name, sp, e, h = key
    vol = named[name]
    d2 = R3.inner_distance(vol, sp, e)
    rep, edges = SR3.basins(vol, d2)
    st = {}
    S3.split_labels3d(vol, h, sp, e, stats=st)
    assert st == dict(basins=len({r for p, r in enumerate(rep) if vol.reshape(-1)[p] > 0}), pairs=len(edges), rounds=reference[key][5],
                      parts=len(reference[key][1]))
    assert st["pairs"] >= 2 and st["rounds"] >= 2 and st["basins"] > st["parts"] >= 1
    with pytest.raises(_lib.UllsamError, match=f"max_pairs = {st['pairs'] - 1}"):
        S3.split_labels3d(vol, h, sp, e, max_pairs=st["pairs"] - 1)
    S3.split_labels3d(vol, h, sp, e, max_pairs=st["pairs"], max_rounds=st["rounds"] + 1)
    with pytest.raises(_lib.UllsamError, match=f"max_rounds = {st['rounds']}"):
        S3.split_labels3d(vol, h, sp, e, max_rounds=st["rounds"])                   # the last round allowed must come to rest


# ---- ABI and resources -------------------------------------------------------------------------------------------------------------------------------
NAMES = {"ullsam_split3d_ascent": 10, "ullsam_split3d_passes": 13, "ullsam_split3d_relabel": 17}


def test_abi_and_symbols():
    from ullsam_amd import build
    build.build(verbose=False)
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "ullsam_hip.h")).read()
    assert _lib.ABI_VERSION == lib.ullsam_abi_version() == int(re.search(r"#define ULLSAM_ABI_VERSION (\d+)", hdr).group(1))
    assert sorted(s for s in _lib.SIGNATURES if s.startswith("ullsam_split3d_")) == sorted(NAMES)
    for s, count in NAMES.items():
        proto = re.search(r"\bint %s\s*\(([^)]*)\)\s*;" % s, hdr)
        assert hasattr(lib, s) and proto, s
        assert len(proto.group(1).split(",")) == count == len(_lib.SIGNATURES[s]), s
        assert len(getattr(lib, s).argtypes) == count, s
    for s in ("ullsam_split_flatten", "ullsam_split_round", "ullsam_split_collect"):          # the flat entry points the volume route reuses
        assert hasattr(lib, s), s


def test_split3d_kernels_have_no_spill_and_no_scratch():
    from ullsam_amd import build
    build.build(verbose=False)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    ks = KR.kernels()
    for pat in KR.HOT_SPLIT3D:
        assert pat in KR.HOT_BF16
    hot = {n: r for n, r in ks.items() if any(re.search(h, n) for h in KR.HOT_SPLIT3D)}
    assert len(hot) == 5, sorted(hot)                                             # four kernels, the ascent in both routes
    assert not any(re.search(h, n) for n in hot for h in KR.HOT_SPLIT)            # (and none of them answers to a 2-D pattern)
    for n, r in hot.items():
        assert not (r.get("vgpr_spill_count", 0) or r.get("sgpr_spill_count", 0) or r.get("private_segment_fixed_size", 0)), (n, r)
    lds = [r.get("group_segment_fixed_size", 0) for n, r in hot.items() if "split3_ascent_kernelILb1E" in n]
    assert lds == [2 * 4 * 66 * 6 * 6]                                            # labels and D2 of 64 x 4 x 4 voxels and their halo
    lds = [r.get("group_segment_fixed_size", 0) for n, r in hot.items() if "split3_passes_kernel" in n]
    assert lds == [3 * 4 * 66 * 6 * 5]                                            # labels, roots and D2 with the forward halo: one plane above
