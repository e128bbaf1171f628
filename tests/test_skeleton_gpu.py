"""Skeletons of label images on the GPU (csrc/skeleton.hip): the device route of utils.skeleton in every route against the host form (itself checked
against the plain loops of tests/skeleton_ref.py without a GPU), the kernels' raw outputs through ops against those loops, the launch-block size, the
measurements, the status word.  Integer work: every assertion is equality."""
import numpy as np
import pytest
import torch

from tests import skeleton_ref as K

pytestmark = pytest.mark.gpu
DEV = "cuda"
DEVICE_ROUTES = ("auto", "global", "lds")


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def N(t):
    return t.cpu().numpy().astype(np.int64)


@pytest.fixture(scope="module")
def shapes():
    from tests.test_skeleton_cpu import shape_list
    return shape_list()


@pytest.fixture(scope="module")
def host(shapes):
    """{name: the host form's Skeleton}: computed once, shared, never changed."""
    from ullsam_amd.utils import skeleton as S
    return {name: S.skeletonize_labels(lab) for name, lab in shapes}


def _same(got, want, what):
    assert got.labels.is_cuda and got.labels.dtype == torch.int32 and tuple(got.labels.shape) == tuple(want.labels.shape), what
    assert torch.equal(got.labels.cpu(), want.labels) and got.subiterations == want.subiterations, (what, got.subiterations, want.subiterations)


@pytest.mark.parametrize("route", DEVICE_ROUTES)
def test_device_route_equals_the_host_form(shapes, host, route):
    from ullsam_amd.utils import skeleton as S
    assert set(DEVICE_ROUTES) == set(S.ROUTES)
    for name, lab in shapes:
        d = T(lab)
        _same(S.skeletonize_labels(d, route=route), host[name], (name, route))
        assert torch.equal(d.cpu(), torch.from_numpy(lab)), (name, "the input was written")
    assert host["a disc of radius 24"].subiterations > 2 * 8                       # more than one LDS launch holds


def test_block_size_numpy_labels_and_two_runs(shapes, host):
    from ullsam_amd import ops
    from ullsam_amd.utils import skeleton as S
    assert ops.SKEL_BLOCK not in (8, 48)
    for name, lab in shapes:
        d = T(lab)
        for route in ("global", "lds"):
            a, b = S.skeletonize_labels(d, route=route, block=8), S.skeletonize_labels(d, route=route, block=48)
            _same(a, host[name], (name, route, 8))
            _same(b, host[name], (name, route, 48))
        _same(S.skeletonize_labels(lab, device=DEV), host[name], (name, "numpy labels, device="))
        x, y = S.skeletonize_labels(d), S.skeletonize_labels(d)
        assert torch.equal(x.labels, y.labels) and x.subiterations == y.subiterations, (name, "two runs differ")
    with pytest.raises(ValueError):
        S.skeletonize_labels(T(shapes[0][1]), block=12)


def test_unaligned_base_pointer(shapes, host):
    from ullsam_amd.utils import skeleton as S
    for name in ("H * W no multiple of 4", "whole rows, width 65", "a disc of radius 24"):
        lab = dict(shapes)[name]
        h, w = lab.shape
        for off in (1, 3):
            flat = torch.zeros((h * w + 8,), dtype=torch.int32, device=DEV)
            flat[off:off + h * w] = T(lab).reshape(-1)
            d = flat[off:off + h * w].view(h, w)
            assert d.is_contiguous() and d.data_ptr() % 16 != 0
            for route in ("global", "lds"):
                _same(S.skeletonize_labels(d, route=route), host[name], (name, off, route))


def test_one_global_sub_iteration_of_each_parity_against_the_loops(shapes):
    from ullsam_amd import ops
    for name, lab in shapes:
        if lab.size > 10000:
            continue
        d = T(lab)
        for index in (0, 1, 6, 7):
            want, deleted = K.subiteration(lab.astype(np.int64), index)
            out, counts, flags = ops.skel_step(d, None, index)
            assert out.dtype == torch.int32 and tuple(out.shape) == lab.shape and np.array_equal(N(out), want), (name, index)
            assert counts.cpu().tolist() == [deleted] and flags.cpu().tolist() == [0, 0, 0, 0], (name, index)
            out2, counts, flags = ops.skel_step(d, torch.empty_like(d), index, limit=index, counts=counts)      # the counter adds; at the limit
            assert torch.equal(out2, out) and counts.cpu().tolist() == [2 * deleted] and flags.cpu().tolist() == [0, int(deleted > 0), 0, 0], (name, index)


def _straddling():
    """A thick disc centred on a corner of the 64 x 32 tiles, a block over a whole row of tiles, a frame-filling instance of 70 x 131."""
    block = np.zeros((45, 150), np.int32)
    block[20:43, 3:147] = 7
    two = np.zeros((70, 131), np.int32)
    two[:, :66] = 1
    two[:, 66:] = 2
    return [("a disc of radius 24", K.disc(70, 131, 32, 64, 24)), ("a block over three tiles", block), ("two instances fill 70 x 131", two)]


def test_one_lds_launch_against_the_loops():
    """SKEL_TILE_STEPS sub-iterations in one launch, with their counters, where a halo one pixel too shallow shows: thick instances across tile corners."""
    from ullsam_amd import ops
    s = ops.SKEL_TILE_STEPS
    assert ops.SKEL_TILE == (32, 64)
    for name, lab in _straddling():
        for index in (0, 1):                                                     # (the driver starts launches at even numbers; the kernel takes any)
            img, want_counts = lab.astype(np.int64), []
            for j in range(s):
                img, deleted = K.subiteration(img, index + j)
                want_counts.append(deleted)
            assert all(c > 0 for c in want_counts), name                         # the front is still moving at the launch's end
            out, counts, flags = ops.skel_tile(T(lab), None, index)
            assert out.dtype == torch.int32 and np.array_equal(N(out), img), (name, index)
            assert counts.cpu().tolist() == want_counts and flags.cpu().tolist() == [0, 0, 0, 0], (name, index)
            cur = T(lab)
            for j in range(s):                                                   # and eight launches of the global kernel say the same
                cur, _, _ = ops.skel_step(cur, None, index + j)
            assert torch.equal(cur, out), (name, index)
            _, counts, flags = ops.skel_tile(T(lab), None, index, limit=index + 3)
            assert counts.cpu().tolist() == want_counts and flags.cpu().tolist() == [0, 1, 0, 0], (name, index)
    empty, counts, flags = ops.skel_tile(torch.zeros((40, 70), dtype=torch.int32, device=DEV), torch.full((40, 70), 9, dtype=torch.int32, device=DEV), 0)
    assert int(empty.abs().sum()) == 0 and counts.cpu().tolist() == [0] * s and flags.cpu().tolist() == [0, 0, 0, 0]


def test_measurements_on_device_equal_the_host_form(shapes, host):
    from ullsam_amd import ops
    from ullsam_amd.utils import distance as D
    from ullsam_amd.utils import skeleton as S
    for name, lab in shapes:
        sk = host[name].labels
        k = int(lab.max())
        for img in (sk, torch.from_numpy(lab)):
            d = img.to(DEV)
            want, got = S.measure_skeletons(img, num_ids=k), S.measure_skeletons(d, num_ids=k)
            for f, g, w in zip(want._fields[:7], got, want):
                assert g.is_cuda and g.dtype == torch.int64 and torch.equal(g.cpu(), w), (name, f)
            assert got.d2_sum is None and torch.equal(S.measure_skeletons(d).pixels.cpu(), want.pixels)
            nodes = S.node_image(d)
            assert nodes.is_cuda and nodes.dtype == torch.uint8 and torch.equal(nodes.cpu(), S.node_image(img)), name
        d2 = D.inner_distance(T(lab))                                            # stays on the device
        assert d2.is_cuda
        got, want = S.measure_skeletons(sk.to(DEV), num_ids=k + 1, d2=d2), S.measure_skeletons(sk, num_ids=k + 1, d2=d2.cpu())
        for f, g, w in zip(want._fields, got, want):
            assert g.is_cuda and g.dtype == w.dtype and torch.equal(g.cpu(), w), (name, f)
    raw, nodes, flags = ops.skel_measure(T(shapes[0][1]), 3, None, nodes=True)
    assert sorted(raw) == sorted(ops.SKEL_FIELDS) and nodes.dtype == torch.uint8 and flags.cpu().tolist() == [0, 0, 0, 0]


def test_too_few_sub_iterations_raise_from_the_status_word_and_the_next_call_works(shapes, host):
    from ullsam_amd import ops
    from ullsam_amd.utils import skeleton as S
    name = "a disc of radius 24"
    d = T(dict(shapes)[name])
    n = host[name].subiterations
    for route in ("global", "lds"):
        for limit in (0, 5, n - 1):
            with pytest.raises(ops._lib.UllsamError) as e:
                S.skeletonize_labels(d, route=route, max_subiterations=limit)
            assert f"max_subiterations = {limit}" in str(e.value)
        _same(S.skeletonize_labels(d, route=route, max_subiterations=n), host[name], ("the next call", route))
    torch.cuda.synchronize()                                                     # (a fault would surface here, and as another error)


def test_a_negative_label_raises_and_the_next_call_works(shapes, host):
    from ullsam_amd import ops
    from ullsam_amd.utils import skeleton as S
    name = "dense blobs, 3 ids, 40 x 29"
    lab = dict(shapes)[name]
    neg = lab.copy()
    neg[0, 0] = -3
    neg[20, 15] = -1
    for route in ("global", "lds"):
        with pytest.raises(ops._lib.UllsamError):
            S.skeletonize_labels(T(neg), route=route)
        _same(S.skeletonize_labels(T(lab), route=route), host[name], ("the next call", route))
    with pytest.raises(ops._lib.UllsamError):
        S.measure_skeletons(T(neg))
    with pytest.raises(ops._lib.UllsamError):
        S.measure_skeletons(T(lab), num_ids=int(lab.max()) - 1)
    with pytest.raises(ops._lib.UllsamError):
        S.node_image(T(neg))
    for bad in (lambda: S.skeletonize_labels(T(lab), route="fast"), lambda: S.skeletonize_labels(T(lab)[0]), lambda: S.skeletonize_labels(T(lab), max_subiterations=-1),
                lambda: S.measure_skeletons(T(lab), d2=T(lab)[:3])):
        with pytest.raises(ValueError):
            bad()
