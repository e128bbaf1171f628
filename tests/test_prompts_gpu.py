"""Prompts from an instance label image on the GPU (csrc/prompts.hip through utils.prompts.prompts_from_labels): every output, the counts and the
two candidate sets (the op's debug images) bit-equal to the brute-force definitions of tests/prompts_ref.py -- frames that are no multiple of any
tile, every branch of the point rules, the choice rule, explicit ids, the fallbacks, a window that spans several workgroups -- and the single
kernels through their ops wrappers (ullsam_label_d1, ullsam_prompt_choose, ullsam_prompt_sets, ullsam_prompt_points, ullsam_instance_masks)."""
import functools

import numpy as np
import pytest
import torch

from tests import prompts_ref as R

pytestmark = pytest.mark.gpu

FIELDS = ("ids", "coords", "point_labels", "boxes", "masks", "counts")

CASES = {
    "a_default": ("scene_a", dict(max_instances=16)),
    "a_radius1": ("scene_a", dict(max_instances=16, inner_radius=1, ring=(1, 2))),
    "a_choice": ("scene_a", dict(max_instances=3, seed=5)),
    "a_ids": ("scene_a", dict(ids=[8, 2, 5], seed=9)),
    "b_cyclic": ("scene_b", dict(num_pos=4, num_neg=2, max_instances=8)),
    "b_radius1": ("scene_b", dict(max_instances=8, inner_radius=1, ring=(1, 2), seed=3)),
    "c_fallback_cyclic": ("scene_c", dict()),
    "d_fallback_outside": ("scene_d", dict()),
    "d_fallback_far": ("scene_d", dict(inner_radius=2, ring=(20, 20))),
    "e_window_of_many_tiles": ("scene_e", dict(num_pos=16, num_neg=16, seed=2 ** 63 + 11)),
}


@functools.lru_cache(maxsize=None)
def _ref(name):
    scene, kw = CASES[name]
    lab = getattr(R, scene)()
    lab.setflags(write=False)
    return lab, R.prompts(lab, **kw)


def _same(ps, ref):
    for f in FIELDS:
        got, want = getattr(ps, f), ref[f]
        assert isinstance(got, torch.Tensor) and got.is_cuda, f
        got = got.cpu().numpy()
        assert got.dtype == want.dtype and got.shape == want.shape, (f, got.dtype, got.shape, want.dtype, want.shape)
        assert np.array_equal(got, want), (f, got if got.size < 200 else None, want if want.size < 200 else None)


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_route_is_bit_equal_to_the_definitions(name):
    from ullsam_amd.utils import prompts as P
    lab, ref = _ref(name)
    kw = CASES[name][1]
    ps = P.prompts_from_labels(torch.from_numpy(np.array(lab)).cuda(), **kw)
    _same(ps, ref)
    for k, i in enumerate(ref["ids"]):
        assert np.array_equal(ps.masks[k].cpu().numpy(), (lab == i).astype(np.float32))
    inner, ring = P.candidate_sets(torch.from_numpy(np.array(lab)).cuda(), ref["ids"], kw.get("inner_radius", 10), kw.get("ring", (9, 11)))
    assert inner.dtype == torch.bool and np.array_equal(inner.cpu().numpy(), ref["inner"])
    assert np.array_equal(ring.cpu().numpy(), ref["ring"])
    again = P.prompts_from_labels(np.array(lab), device="cuda", **kw)        # numpy labels with a device: the same kernels, the same bytes
    for f in FIELDS:
        assert getattr(again, f).cpu().numpy().tobytes() == getattr(ps, f).cpu().numpy().tobytes(), f


def test_scenes_cover_what_they_are_meant_to():
    a = _ref("a_default")[1]
    assert a["ids"].tolist() == [1, 2, 3, 5, 7, 8] and a["counts"][0, 0] > 0 and a["counts"][1, 0] == 0 and a["counts"][2, 0] == 0
    assert _ref("a_choice")[1]["ids"].tolist() not in ([1, 2, 3], []) and len(_ref("a_choice")[1]["ids"]) == 3
    assert _ref("b_cyclic")[1]["counts"][0, 0] == 3
    assert _ref("c_fallback_cyclic")[1]["counts"][0, 1] == 0 and _ref("d_fallback_outside")[1]["counts"][0, 1] == 1
    assert _ref("d_fallback_far")[1]["counts"][0, 1] == 0
    e = _ref("e_window_of_many_tiles")[1]
    assert e["boxes"][0].tolist() == [40, 50, 240, 250] and e["counts"][0, 0] > 16 and e["counts"][0, 1] > 16


def test_empty_image_absent_id_and_bad_labels():
    from ullsam_amd.utils import prompts as P
    z = torch.zeros((64, 48), dtype=torch.int32, device="cuda")
    ps = P.prompts_from_labels(z, num_pos=2, num_neg=5)
    _same(ps, R.prompts(np.zeros((64, 48), np.int32), num_pos=2, num_neg=5))
    lab = torch.from_numpy(R.scene_a()).cuda()
    with pytest.raises(ValueError, match="id 4 has no pixels"):
        P.prompts_from_labels(lab, ids=[1, 4])
    with pytest.raises(ValueError, match="0..65535"):
        P.prompts_from_labels(lab + 65530)
    with pytest.raises(ValueError, match="fills the frame"):
        P.prompts_from_labels(torch.full((40, 50), 2, dtype=torch.int32, device="cuda"))
    assert P.prompts_from_labels(lab, return_masks=False).masks is None
    assert P.prompts_from_labels(lab, ids=torch.tensor([7], device="cuda")).ids.tolist() == [7]


def test_arguments_are_checked_up_front():
    """Labels wider than int32 cannot wrap into range, narrower ones are taken as they are, and the slots are bounded by their scratch memory."""
    from ullsam_amd.utils import prompts as P
    lab, ref = _ref("a_default")
    wide = torch.from_numpy(lab.astype(np.int64)).cuda()
    _same(P.prompts_from_labels(wide, max_instances=16), ref)
    with pytest.raises(ValueError, match="0..65535"):
        P.prompts_from_labels(wide + 2 ** 32)                                    # int32(2^32 + 1) would be the disc's id
    with pytest.raises(ValueError, match="0..65535"):
        P.prompts_from_labels(lab.astype(np.int64) + 2 ** 32, device="cuda")
    with pytest.raises(ValueError, match="id 65536 has no pixels"):
        P.prompts_from_labels(wide, ids=torch.tensor([2 ** 32 + 1]))
    small = np.where(lab > 0, lab + 200, 0).astype(np.uint8)                     # ids 201..208: above int8's range
    ps = P.prompts_from_labels(torch.from_numpy(small).cuda(), ids=[201, 208])
    assert np.array_equal(ps.counts.cpu().numpy(), ref["counts"][[0, 5]]) and np.array_equal(ps.boxes.cpu().numpy(), ref["boxes"][[0, 5]])
    with pytest.raises(ValueError, match="GiB of device scratch"):
        P.prompts_from_labels(torch.zeros((1024, 1024), dtype=torch.int32, device="cuda"), max_instances=65535)
    with pytest.raises(ValueError, match="<= 64"):
        P.prompts_from_labels(wide, ring=(9, 65))


def test_kernels_through_their_wrappers():
    """The chain utils.prompts runs, kernel by kernel, on scene b (160 x 96) with radius 3 and ring (2, 4)."""
    from ullsam_amd import ops
    from ullsam_amd.utils import prompts as P
    lab = R.scene_b()
    t = torch.from_numpy(lab).cuda()
    d1, status = ops.label_d1(t, 3)
    assert d1.dtype == torch.uint8 and np.array_equal(d1.cpu().numpy(), np.minimum(R.d1(lab), 4)) and int(status) == 0
    assert int(ops.label_d1(t - 1, 3)[1]) == 1                                   # a negative label is reported
    areas, boxes_t = ops.label_stats(t, ops.PROMPT_MAX_ID)
    sel, info = ops.prompt_choose(areas, 8, 0)
    assert int(info[0]) == 4 and sel[:4].tolist() == [2, 4, 11, 65535]
    sel2, info2 = ops.prompt_choose(areas, 2, 7)
    assert int(info2[0]) == 2 and sel2.tolist() == R.choose(lab, 2, 7) == P.choose_instances([2, 4, 11, 65535], 2, 7).tolist()
    bits, rowcnt, sums, dbg = ops.prompt_sets(t, d1, areas, boxes_t, sel, info, 3, (2, 4), debug=True)
    ref = R.prompts(lab, num_pos=2, num_neg=3, max_instances=8, inner_radius=3, ring=(2, 4), seed=1)
    assert np.array_equal(dbg[0][:4].cpu().numpy().astype(bool), ref["inner"]) and np.array_equal(dbg[1][:4].cpu().numpy().astype(bool), ref["ring"])
    assert not dbg[0][4:].any() and not dbg[1][4:].any()                         # the slots past info[0] stay empty
    assert np.array_equal(rowcnt[0, :4].cpu().numpy(), ref["inner"].sum(2)) and np.array_equal(rowcnt[1, :4].cpu().numpy(), ref["ring"].sum(2))
    for k, i in enumerate(ref["ids"]):
        ys, xs = np.where(lab == i)
        assert sums[k].tolist() == [int(xs.sum()), int(ys.sum())]
    coords, boxes, counts = ops.prompt_points(lab.shape, areas, boxes_t, sel, info, bits, rowcnt, sums, 4, 2, 3, 1)
    assert np.array_equal(coords[:4].cpu().numpy(), ref["coords"]) and np.array_equal(boxes[:4].cpu().numpy(), ref["boxes"])
    assert np.array_equal(counts[:4].cpu().numpy(), ref["counts"]) and not coords[4:].any()
    rec = info.cpu().numpy()[2:18].reshape(4, 4)
    assert rec[:, 0].tolist() == [2, 4, 11, 65535] and np.array_equal(rec[:, 2:], ref["counts"]) and rec[:, 1].tolist() == [int((lab == i).sum()) for i in ref["ids"]]
    masks = ops.instance_masks(t, sel[:4].contiguous())
    assert masks.dtype == torch.float32 and np.array_equal(masks.cpu().numpy(), ref["masks"])
    with pytest.raises(Exception):
        ops.label_d1(t, 65)
