"""The interactive loop on the GPU: the finish kernel (ops.click_finish) against its host form bit for bit, its mask against the existing resize
kernel, and the InteractiveSegmenter session on the tiny composite -- one encoder pass per image, logits equal to the model API's, canvas and
overlay equal to the host form's, and the device-resident chain prompts_from_labels -> predict_instances -> label_overlap."""
import numpy as np
import pytest
import torch

from oracle import ullsam_oracle as O
from tests import interactive_ref as R
from tests import util as U
from ullsam_amd.utils import interactive as I

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 0xA5
PAD = 64


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _guarded(shape, dtype, fill=None):
    """A tensor of `shape` inside a larger buffer whose PAD elements before and after it hold a sentinel."""
    n = int(np.prod(shape))
    s = SENT if dtype == torch.uint8 else 0x5A5A5A5A
    buf = torch.full((n + 2 * PAD,), s, dtype=dtype, device=DEV)
    view = buf[PAD:PAD + n].view(*shape)
    if fill is not None:
        view.copy_(fill)
    return buf, view, s


def _borders_intact(buf, s):
    return bool((buf[:PAD] == s).all()) and bool((buf[-PAD:] == s).all())


def _run(ops, low, S, hw, side, top, left, thr, image, canvas, first_id, paint, highlight, luts):
    P = low.shape[0]
    mb, mask, ms = _guarded((P,) + tuple(hw), torch.uint8)
    ob, overlay, os_ = _guarded(tuple(hw) + (3,), torch.uint8)
    sb, stats, ss = _guarded((P, 5), torch.int32)
    cb, cv, cs = _guarded(tuple(hw), torch.int32, fill=T(canvas))
    ops.click_finish(T(low), S, hw, side, top, left, thr, image=T(image), canvas=cv, first_id=first_id, paint=paint, highlight=highlight,
                     lut_inst=luts[0], lut_cur=luts[1], mask=mask, overlay=overlay, stats=stats)
    torch.cuda.synchronize()
    for b, s in ((mb, ms), (ob, os_), (sb, ss), (cb, cs)):
        assert _borders_intact(b, s), "a write outside an output buffer"
    return mask.cpu().numpy(), cv.cpu().numpy(), overlay.cpu().numpy(), stats.cpu().numpy()


@pytest.fixture(scope="module")
def ops():
    from ullsam_amd import ops as o
    return o


@pytest.fixture(scope="module")
def luts():
    return tuple(T(a) for a in I.blend_luts(R.TEST_PALETTE)), I.blend_luts(R.TEST_PALETTE)


@pytest.mark.parametrize("name", ["p1", "p3", "p3_full_empty"])
@pytest.mark.parametrize("shape", list(R.SHAPES))
def test_click_finish_equals_the_host_form(ops, luts, shape, name):
    """Every input set (one mask; three overlapping ones with logits of exactly 0.0 and +-1e-30; full / empty / blob) under every flag combination,
    on a canvas whose ids run far beyond the palette: mask, canvas, overlay and stats equal the host form's bits, twice, and nothing is written
    outside the outputs."""
    n, S, hw, side, top, left = R.SHAPES[shape]
    image, canvas = R.display_inputs(hw)
    dev_luts, host_luts = luts
    low = R.lows(n)[name]
    for paint, highlight in R.FLAGS:
        args = (low, S, hw, side, top, left, 0.0, image, canvas, 50, paint, highlight)
        ids = canvas.copy()
        hm, ho, hs = I.click_finish_host(low, S, hw, side, top, left, 0.0, image=image, canvas=ids, first_id=50, paint=paint, highlight=highlight,
                                         lut_inst=host_luts[0], lut_cur=host_luts[1], want_overlay=True)
        got = _run(ops, *args, dev_luts)
        for what, g, r in zip(("mask", "canvas", "overlay", "stats"), got, (hm, ids, ho, hs)):
            assert g.dtype == r.dtype and np.array_equal(g, r), (shape, name, paint, highlight, what, int((g != r).sum()))
        again = _run(ops, *args, dev_luts)
        assert all(np.array_equal(a, b) for a, b in zip(got, again)), (shape, name, paint, highlight, "two runs differ")


@pytest.mark.parametrize("shape", ["portrait_pad", "off_size"])
def test_click_finish_outputs_are_optional(ops, luts, shape):
    """Each output alone gives the bits it has among all of them; an output not asked for is not touched (None comes back), the canvas of a call
    that does not paint keeps its bits, and another threshold is honoured."""
    n, S, hw, side, top, left = R.SHAPES[shape]
    image, canvas = R.display_inputs(hw)
    low = R.lows(n)["p3"]
    dl = luts[0]
    full = _run(ops, low, S, hw, side, top, left, 0.25, image, canvas, 7, True, True, dl)
    cv = T(canvas)
    m, o, s = ops.click_finish(T(low), S, hw, side, top, left, 0.25, want_mask=True, want_stats=False)
    assert o is None and s is None and np.array_equal(m.cpu().numpy(), full[0])
    m, o, s = ops.click_finish(T(low), S, hw, side, top, left, 0.25, want_mask=False, want_stats=True)
    assert m is None and o is None and np.array_equal(s.cpu().numpy(), full[3])
    m, o, s = ops.click_finish(T(low), S, hw, side, top, left, 0.25, image=T(image), canvas=cv, first_id=7, paint=True, highlight=True, lut_inst=dl[0],
                               lut_cur=dl[1], want_mask=False, want_overlay=True, want_stats=False)
    assert m is None and s is None and np.array_equal(o.cpu().numpy(), full[2]) and np.array_equal(cv.cpu().numpy(), full[1])
    hm, _, hs = I.click_finish_host(low, S, hw, side, top, left, 0.25)
    assert np.array_equal(full[0], hm) and np.array_equal(full[3], hs)


@pytest.mark.parametrize("shape", list(R.SHAPES))
def test_mask_equals_the_resize_kernel_gathered_at_the_nearest_index(ops, shape):
    from ullsam_amd.utils.amg import nearest_source_index
    n, S, hw, side, top, left = R.SHAPES[shape]
    low = T(R.lows(n)["p3"])
    for thr in (0.0, -0.5):
        _, up = ops.resize_bilinear(low, (S, S), want_float=False, threshold=thr)
        iy = T(nearest_source_index(side, S)[top:top + hw[0]])
        ix = T(nearest_source_index(side, S)[left:left + hw[1]])
        mask, _, _ = ops.click_finish(low, S, hw, side, top, left, thr, want_stats=False)
        assert torch.equal(mask, up[:, iy][:, :, ix]), (shape, thr)


def test_click_finish_checks_its_arguments(ops, luts):
    from ullsam_amd._lib import UllsamError
    low = torch.zeros((1, 8, 8), device=DEV)
    with pytest.raises(UllsamError, match="window"):
        ops.click_finish(low, 32, (8, 8), 8, 1, 0)
    with pytest.raises(UllsamError, match="window"):
        ops.click_finish(low, 32, (8, 8), 8, 0, -1)
    with pytest.raises(UllsamError, match="positive"):
        ops.click_finish(low, 0, (8, 8))
    with pytest.raises(UllsamError, match="positive"):
        ops.click_finish(torch.zeros((0, 8, 8), device=DEV), 32, (8, 8))
    with pytest.raises(UllsamError, match="overlay"):
        ops.click_finish(low, 32, (8, 8), want_overlay=True)
    with pytest.raises(UllsamError, match="canvas"):
        ops.click_finish(low, 32, (8, 8), paint=True)
    with pytest.raises(UllsamError, match="K >= 1"):
        ops.click_finish(low, 32, (8, 8), image=torch.zeros((8, 8, 3), dtype=torch.uint8, device=DEV), lut_inst=torch.zeros((0, 3, 256), dtype=torch.uint8, device=DEV),
                         lut_cur=luts[0][1], want_overlay=True)


# ---- the session on the tiny composite ------------------------------------------------------------------------------------------------
def _load(module, P, dtype):
    sd = {k: torch.from_numpy(v) for k, v in P.items()}
    missing, unexpected = module.load_state_dict(sd, strict=False)
    assert not missing and not unexpected, (missing[:3], unexpected[:3])
    return module.to(DEV).to(dtype).eval()


def _ullsam_tiny(dtype):
    from ullsam_amd.build_sam import _build_sam
    from ullsam_amd.modeling.configuration_internvl_chat import InternVLChatConfig
    from ullsam_amd.modeling.modeling_internvl_sam import InternVLSAMModel
    c = U.LLM_TINY
    sam = _build_sam(128, 2, 2, [1])
    cfg = InternVLChatConfig(vision_config={"architectures": ["SAM-ViT-B-16"]},
                             llm_config=dict(architectures=["InternLM2ForCausalLM"], vocab_size=c["vocab"], hidden_size=c["hidden"],
                                             intermediate_size=c["inter"], num_hidden_layers=c["layers"], num_attention_heads=c["heads"],
                                             num_key_value_heads=c["kv_heads"], bias=False, max_position_embeddings=32768,
                                             rope_theta=c["rope_theta"], rms_norm_eps=c["eps"]),
                             downsample_ratio=0.5, template="internlm2-chat", ps_version="v2", force_image_size=1024)
    m = InternVLSAMModel(cfg, vision_model=sam.image_encoder, prompt_encoder=sam.prompt_encoder, mask_decoder=sam.mask_decoder)
    return _load(m, U.ullsam_tiny_params(0), dtype)


CLICKS = ([[512, 384]], [[200, 830]], [[760, 620], [300, 300]])          # display pixels (x, y) on the 1024^2 image: frame pixels too
CLICK_LABELS = ([1], [1], [1, 0])


class _Session:
    """One model, one image, one session per dtype; the encoders' forwards are counted from the start."""

    def __init__(self, dtype):
        from ullsam_amd.interactive import InteractiveSegmenter
        self.dtype = dtype
        self.m = m = _ullsam_tiny(dtype)
        self.calls = {"vit": 0, "llm": 0}
        vit_tokens, llm_forward = m.vision_model.forward_tokens, m.language_model.forward

        def vit(*a, **k):
            self.calls["vit"] += 1
            return vit_tokens(*a, **k)

        def llm(*a, **k):
            self.calls["llm"] += 1
            return llm_forward(*a, **k)

        m.vision_model.forward_tokens, m.language_model.forward = vit, llm
        self.image = np.random.default_rng(11).integers(0, 256, (1024, 1024, 3), dtype=np.uint8)
        self.ids = torch.from_numpy(O.make_input_ids(20, 34, seed=3)).to(DEV)
        self.seg = InteractiveSegmenter(m, self.ids, palette=R.TEST_PALETTE)
        self.seg.set_image(self.image)
        self.after_set_image = dict(self.calls)
        self.results, self.cache_has_keys = [], []
        for pts, lbl in zip(CLICKS, CLICK_LABELS):
            self.results.append(self.seg.click(pts, lbl))
            self.cache_has_keys.append("keys" in self.seg.image_cache)
        self.after_clicks = dict(self.calls)

    def api(self, pts, lbl, use_llm=True, mask_input=None):
        """The model API on the same frame coordinates (app.py:580-633): forward, prompt encoder, mask decoder."""
        from ullsam_amd.utils.imageprep import preprocess_image
        m = self.m
        x = preprocess_image(self.image, device=DEV).to(self.dtype)
        out = m(pixel_values=x, input_ids=self.ids, attention_mask=torch.ones_like(self.ids), image_flags=(self.ids == 92546)[..., None].long(),
                return_dict=True, use_cache=False, output_hidden_states=True)
        p = torch.tensor([pts], dtype=torch.float32, device=DEV)
        l = torch.tensor([lbl], dtype=torch.int32, device=DEV)
        sp, de = m.prompt_encoder(points=(p, l), boxes=None, masks=mask_input, llm_hidden_states=out.hidden_states if use_llm else None)
        return m.mask_decoder(image_embeddings=out.image_embeddings, image_pe=m.prompt_encoder.get_dense_pe(), sparse_prompt_embeddings=sp,
                              dense_prompt_embeddings=de, multimask_output=False)


_SESSIONS = {}


@pytest.fixture(params=[torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def ses(request):
    if request.param not in _SESSIONS:
        _SESSIONS[request.param] = _Session(request.param)
    return _SESSIONS[request.param]


def test_session_runs_the_encoders_once_per_image(ses):
    assert ses.after_set_image == {"vit": 1, "llm": 1}
    assert ses.after_clicks == {"vit": 1, "llm": 1}, "a click ran an encoder"
    assert ses.cache_has_keys == [True, True, True], "the decoder's image-side cache did not survive the clicks"
    src = ses.seg.image_cache["_source"]
    assert src[0] is ses.seg.image_tokens and src[1] is ses.seg.dense


def _close(got, want, what, dtype):
    """The logits of the session against the model API's: the same kernels on the same values, so a bf16 model's are held bit-equal.  In fp32 one
    kernel differs: the session asks the decoder for the one mask it needs (mask_range), the API computes all four and slices, and the compiler
    unrolled hyper_masks_kernel's loop over masks by two with a remainder body it contracts differently (DESIGN.md "7b, continued: the interactive
    loop") -- last-bit differences, at most 4.8e-7 measured, held to the bound of test_batched_forward_equals_per_sample: 2e-4 on the logits, mask
    mismatch share below 1e-5."""
    d = (got - want).abs().max().item()
    mism = ((got > 0) != (want > 0)).float().mean().item()
    print(f"{what} {dtype}: max |session - api| = {d:.3e}, mask mismatch share = {mism:.3e}, bit-equal = {torch.equal(got, want)}")
    assert got.dtype == torch.float32 and got.shape == want.shape
    if dtype == torch.bfloat16:
        assert torch.equal(got, want), (what, d, mism)
    else:
        assert d < 2e-4 and mism < 1e-5, (what, d, mism)


def test_click_logits_equal_the_model_api(ses):
    """The model API on the same frame coordinates gives the session's logits and IoU predictions, and at a 1024^2 display the mask is the
    upsampled logits' sign."""
    from ullsam_amd import ops
    before = ses.calls["vit"]
    for r, pts, lbl in zip(ses.results, CLICKS, CLICK_LABELS):
        low, iou = ses.api(pts, lbl)
        assert tuple(r.low.shape) == (1, 1, 256, 256)
        _close(r.low, low, f"click {pts}", ses.dtype)
        assert torch.equal(r.iou, iou[0]), (pts, r.iou, iou)
        _, up = ops.resize_bilinear(r.low[:, 0].contiguous(), (1024, 1024), want_float=False, threshold=0.0)
        assert r.mask.dtype == torch.uint8 and torch.equal(r.mask, up[0])
        m = r.mask.cpu().numpy()
        ys, xs = np.nonzero(m)
        want = [0, 0, 0, 0] if ys.size == 0 else [xs.min(), ys.min(), xs.max(), ys.max()]
        assert int(r.area) == int(m.sum()) and r.box.cpu().tolist() == [int(v) for v in want]
    assert ses.calls["vit"] - before == len(CLICKS), "the API route encodes once per click (what the session saves)"


def test_baseline_mode_and_mask_input_equal_the_model_api(ses):
    from ullsam_amd.interactive import InteractiveSegmenter
    base = InteractiveSegmenter(ses.m, ses.ids, use_llm_prompt=False)
    base.set_image(ses.image)
    r = base.click(CLICKS[0], CLICK_LABELS[0])
    low, iou = ses.api(CLICKS[0], CLICK_LABELS[0], use_llm=False)
    _close(r.low, low, "baseline mode", ses.dtype)
    assert torch.equal(r.iou, iou[0])
    assert (r.low - ses.results[0].low).abs().max().item() > 1e-3, "the LLM prompt must change the logits"
    prev = ses.results[0].low
    low_s, iou_s = ses.seg.predict([CLICKS[1]], [CLICK_LABELS[1]], mask_input=prev)
    low_a, iou_a = ses.api(CLICKS[1], CLICK_LABELS[1], mask_input=prev)
    _close(low_s, low_a, "mask_input", ses.dtype)
    assert torch.equal(iou_s, iou_a)
    assert (low_s - ses.results[1].low).abs().max().item() > 1e-3, "the mask input must change the logits"
    assert "keys" in ses.seg.image_cache, "a mask_input call must leave the session's cache alone"
    low3, iou3 = ses.seg.predict([CLICKS[0]], [CLICK_LABELS[0]], multimask_output=True)
    assert tuple(low3.shape) == (1, 3, 256, 256) and tuple(iou3.shape) == (1, 3)
    low4, iou4 = ses.m.mask_decoder.predict_masks_tokens(ses.seg.image_tokens, ses.seg.dense_pe, ses.m.prompt_encoder.sparse_tokens(
        (torch.tensor([CLICKS[0]], dtype=torch.float32, device=DEV), torch.tensor([CLICK_LABELS[0]], dtype=torch.int32, device=DEV)), None), ses.seg.dense, (64, 64))
    _close(low3, low4[:, 1:], "multimask", ses.dtype)
    assert torch.equal(iou3, iou4[:, 1:])


def test_canvas_and_overlays_equal_the_host_form(ses):
    """Three click + save_instance rounds with overlapping masks against the host form run on the downloaded logits; then predict_instances with the
    same prompts against the rounds, export_labels and reset_instances."""
    seg = ses.seg
    seg.reset_instances()
    lut_inst, lut_cur = I.blend_luts(R.TEST_PALETTE)
    canvas = np.zeros((1024, 1024), np.int32)
    singles = []
    for k, (pts, lbl) in enumerate(zip(CLICKS, CLICK_LABELS)):
        r = seg.click(pts, lbl)
        low = r.low[0].cpu().numpy()
        singles.append(r)
        hm, ho, hs = I.click_finish_host(low, 1024, (1024, 1024), image=ses.image, canvas=canvas, highlight=True, lut_inst=lut_inst, lut_cur=lut_cur,
                                         want_overlay=True)
        assert np.array_equal(r.mask.cpu().numpy(), hm[0]) and np.array_equal(r.overlay.cpu().numpy(), ho), k
        assert [int(r.area)] + r.box.cpu().tolist() == hs[0].tolist()
        assert torch.equal(seg.render(), r.overlay) and torch.equal(seg.current_mask, r.mask)
        over = seg.save_instance()
        _, ho, _ = I.click_finish_host(low, 1024, (1024, 1024), image=ses.image, canvas=canvas, first_id=k + 1, paint=True, lut_inst=lut_inst,
                                       lut_cur=lut_cur, want_overlay=True)
        assert seg.count == k + 1 and seg.current_mask is None
        assert np.array_equal(seg.labels.cpu().numpy(), canvas) and np.array_equal(over.cpu().numpy(), ho), k
        assert torch.equal(seg.render(), over) and torch.equal(seg.render(highlight=False), over)
    masks = np.stack([r.mask.cpu().numpy() for r in singles])
    assert (masks.sum(0) > 1).any(), "the three masks must overlap for the paint order to matter"
    with pytest.raises(RuntimeError):
        seg.save_instance()
    out = seg.export_labels()
    assert out.dtype == np.uint16 and out.shape == (1024, 1024) and np.array_equal(out, canvas)

    # three prompts of one point each, as rounds and in one call
    seg.reset_instances()
    assert seg.count == 0 and not seg.labels.any() and seg.current_mask is None
    one_point = [CLICKS[0], CLICKS[1], CLICKS[2][:1]]
    one_label = [CLICK_LABELS[0], CLICK_LABELS[1], CLICK_LABELS[2][:1]]
    for pts, lbl in zip(one_point, one_label):
        seg.click(pts, lbl)
        seg.save_instance()
    rounds = seg.labels.clone()
    single_low = torch.cat([seg.predict([p], [l])[0] for p, l in zip(one_point, one_label)])
    seg.reset_instances()
    ids, iou, area, box = seg.predict_instances(one_point, one_label)
    batch_low, _ = seg.predict(one_point, one_label)
    d = (batch_low - single_low).abs().max().item()
    mism = ((batch_low > 0) != (single_low > 0)).float().mean().item()
    print(f"predict_instances: max |batched - single| logits = {d:.3e}, low-resolution mask mismatch share = {mism:.3e}")
    assert d < 2e-4 and mism < 1e-5
    assert ids.tolist() == [1, 2, 3] and seg.count == 3 and tuple(iou.shape) == (3,) and tuple(box.shape) == (3, 4)
    _, _, hs = I.click_finish_host(batch_low[:, 0].cpu().numpy(), 1024, (1024, 1024))
    assert torch.equal(torch.cat([area[:, None], box], 1).cpu(), torch.from_numpy(hs))
    want = np.zeros((1024, 1024), np.int32)                  # whatever the decoder gave: the canvas is the host form's paint of these logits
    I.click_finish_host(batch_low[:, 0].cpu().numpy(), 1024, (1024, 1024), canvas=want, first_id=1, paint=True)
    assert np.array_equal(seg.labels.cpu().numpy(), want)
    # these three prompts' batched masks equal their single-prompt masks (the logits came out bit-equal on an MI355X), so one launch must leave
    # what the three save_instance rounds left
    assert torch.equal(_display_masks(batch_low), _display_masks(single_low)), "choose prompts whose batched masks equal the single-prompt ones"
    assert torch.equal(seg.labels, rounds), "one launch must leave what three save_instance rounds leave"
    # more prompts than one finish launch takes: the launches are chained, a later chunk on top
    one_launch = (seg.labels.clone(), area.clone(), box.clone())
    seg.reset_instances()
    from ullsam_amd import ops
    cap = ops.CLICK_MAX_P
    ops.CLICK_MAX_P = 2
    try:
        ids2, _, area2, box2 = seg.predict_instances(one_point, one_label)
    finally:
        ops.CLICK_MAX_P = cap
    assert ids2.tolist() == [1, 2, 3] and torch.equal(seg.labels, one_launch[0]) and torch.equal(area2, one_launch[1]) and torch.equal(box2, one_launch[2])
    seg.count = 65536
    with pytest.raises(ValueError, match="uint16"):
        seg.export_labels()
    seg.reset_instances()
    assert not seg.labels.any() and seg.count == 0


def _display_masks(low):
    from ullsam_amd import ops
    return ops.resize_bilinear(low[:, 0].contiguous(), (1024, 1024), want_float=False, threshold=0.0)[1]


def test_non_square_image_is_unpadded(ses):
    """A 600 x 1024 landscape image: the model sees the centred pad, the session's outputs are the window, and clicks map through the pad."""
    from ullsam_amd.interactive import InteractiveSegmenter
    from ullsam_amd import ops
    seg = InteractiveSegmenter(ses.m, ses.ids, palette=R.TEST_PALETTE)
    grey = np.random.default_rng(5).integers(0, 65536, (600, 1024)).astype(np.uint16)
    seg.set_image(grey)
    assert (seg.H, seg.W, seg.side, seg.top, seg.left) == (600, 1024, 1024, 212, 0)
    assert tuple(seg.image.shape) == (600, 1024, 3) and torch.equal(seg.image[..., 0], seg.image[..., 2])
    r = seg.click([[500, 300]], [1])
    assert tuple(r.mask.shape) == (600, 1024) and tuple(r.overlay.shape) == (600, 1024, 3)
    _, up = ops.resize_bilinear(r.low[:, 0].contiguous(), (1024, 1024), want_float=False, threshold=0.0)
    assert torch.equal(r.mask, up[0, 212:812])
    p = torch.tensor([[[500.0, 512.0]]], device=DEV)
    sp = ses.m.prompt_encoder.sparse_tokens((p, torch.ones((1, 1), dtype=torch.int32, device=DEV)), None)
    low, _ = ses.m.mask_decoder.predict_masks_tokens(seg.image_tokens, seg.dense_pe, sp, seg.dense, (64, 64), mask_range=(0, 1))
    assert torch.equal(r.low, low)
    # a box maps per corner through the pad: (x0, y0, x1, y1) in display pixels -> rows + 212; the last display pixel stays inside the frame
    box = [100, 50, 1023, 599]
    rb = seg.click(boxes=box)
    fb = torch.tensor([[100.0, 50.0 + 212, 1023.0, 599.0 + 212]], device=DEV)
    sp, _ = ses.m.prompt_encoder(points=None, boxes=fb, masks=None, llm_hidden_states=None)
    low, iou = ses.m.mask_decoder.predict_masks_tokens(seg.image_tokens, seg.dense_pe, sp, seg.dense, (64, 64), mask_range=(0, 1))
    assert torch.equal(rb.low, low) and torch.equal(rb.iou, iou[0]) and not torch.equal(rb.low, r.low)
    low_pb, _ = seg.predict([[[500, 300]]], [[1]], boxes=[box])                      # points and a box in one prompt
    sp = ses.m.prompt_encoder.sparse_tokens((p, torch.ones((1, 1), dtype=torch.int32, device=DEV)), fb)
    low, _ = ses.m.mask_decoder.predict_masks_tokens(seg.image_tokens, seg.dense_pe, sp, seg.dense, (64, 64), mask_range=(0, 1))
    assert torch.equal(low_pb, low)
    seg.reset_instances()
    ids, _, area, _ = seg.predict_instances(None, None, boxes=[box, [0, 0, 300, 200]])
    assert ids.tolist() == [1, 2] and seg.count == 2
    low2, _ = seg.predict(boxes=[box, [0, 0, 300, 200]])
    want = np.zeros((600, 1024), np.int32)
    _, _, hs = I.click_finish_host(low2[:, 0].cpu().numpy(), 1024, (600, 1024), 1024, 212, 0, canvas=want, first_id=1, paint=True)
    assert np.array_equal(seg.labels.cpu().numpy(), want) and area.cpu().tolist() == hs[:, 0].tolist()


def test_chain_from_label_image_to_overlap_table_stays_on_the_device(ses):
    """prompts_from_labels -> predict_instances -> label_overlap on device tensors.  One host round trip remains inside predict: the prompt
    coordinates (a few numbers) are mapped to the frame in Python floats on the host, as the app maps a click, and uploaded again; masks, canvas and
    the overlap table never leave the device.  No accuracy claim (random weights): the overlap table's row sums are the painted areas."""
    from ullsam_amd.interactive import InteractiveSegmenter
    from ullsam_amd.utils import amg, prompts, synthetic
    gt = torch.from_numpy(synthetic.label_tile(3, size=128, n_cells=6, r_range=(10.0, 22.0))).to(DEV)
    image = ((gt > 0).to(torch.uint8) * 150 + 40)
    seg = InteractiveSegmenter(ses.m, ses.ids)
    seg.set_image(image)
    ps = prompts.prompts_from_labels(gt, num_pos=1, num_neg=1, max_instances=4, seed=1, inner_radius=3, ring=(3, 5), device=DEV, return_masks=False)
    assert ps.coords.is_cuda and ps.coords.shape[0] >= 2
    ids, iou, area, box = seg.predict_instances(ps.coords, ps.point_labels)
    n = ps.coords.shape[0]
    assert ids.is_cuda and area.is_cuda and seg.labels.is_cuda and seg.count == n and ids.tolist() == list(range(1, n + 1))
    table = amg.label_overlap(seg.labels, gt, na=n, nb=int(gt.max()))
    assert table.is_cuda and tuple(table.shape) == (n + 1, int(gt.max()) + 1)
    painted = torch.bincount(seg.labels.reshape(-1).long(), minlength=n + 1)
    assert torch.equal(table.sum(1), painted) and int(table.sum()) == 128 * 128
    assert bool((painted[1:] <= area.long()).all()) and int(painted[n]) == int(area[n - 1]), "the last prompt lies on top"
    low, _ = seg.predict(ps.coords, ps.point_labels)
    want = np.zeros((128, 128), np.int32)
    I.click_finish_host(low[:, 0].cpu().numpy(), 1024, (128, 128), canvas=want, first_id=1, paint=True)
    assert np.array_equal(seg.labels.cpu().numpy(), want)
