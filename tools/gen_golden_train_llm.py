"""Generate the fixtures of the LLM-training tests (tests/test_train_llm_gpu.py) by running the REFERENCE itself (imported from /root/reference).

Run in the build container only (the reference never travels to the GPU box):
    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_train_llm.py [case ...]

    train_sft_step       the caption trainer's SFT step (train.py:284-318 as train.py:983-984 runs it: --freeze_vision only) on the tiny composite
    train_step_llm       the joint trainer's segmentation step with every module trainable (train_joint_v2.py:1334-1351, loss = 0 * llm_loss + seg_loss)
    train_sft_step_real  the SFT step with one 7B-shaped InternLM2 layer (hidden 4096, 32 / 8 heads, vocab 92553) behind the ViT-B-width SAM

Weights come from oracle.ullsam_oracle.fill_param (seeded, regenerable without the reference); the inputs are built here and stored.  Each
gradient is kept as a strided sample plus its L2 norm, as train_step.npz.  The archives are written with fixed zip timestamps, so that two runs
give the same bytes.
"""
from __future__ import annotations

import io
import os
import sys
import time
import types
import zipfile

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.dont_write_bytecode = True

from oracle import gen_golden as GG  # noqa: E402  (puts /root/reference on sys.path)
from oracle.gen_golden import LLM_7B_L1, LLM_TINY, _sam_small, fill_module, fill_module_inplace, rand_image  # noqa: E402
from oracle import ullsam_oracle as O  # noqa: E402

IMG_CONTEXT = 92546
REPEATED_ID = 777          # a text token that occurs nine times
ABSENT_ID = 50000          # a token id that does not occur
PAD_FILL_ID = 2            # right padding of the SFT dataset (attention_mask 0; the labels keep these ids, train.py:240-275)
STORED_ROWS = (REPEATED_ID, 0, IMG_CONTEXT, ABSENT_ID)


def save(name, **kw):
    """np.savez_compressed with fixed member timestamps (numpy stamps each member with the current time: two runs would differ)."""
    path = os.path.join(GG.OUT, name + ".npz")
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k, v in kw.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(zi, buf.getvalue())
    print(f"  wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


def sft_ids():
    """One SFT sample as train.py's dataset builds it (train.py:240-275), S = 1081: bos, system / user text (with id-0 tokens and a repeated token),
    <img>, 1024 x <IMG_CONTEXT>, </img>, user text, <|im_start|> 'ass' 'istant', the answer (the repeated token again, an id 0), <|im_end|>, then right
    padding with attention_mask 0.  labels = ids with -100 before the assistant turn; the padded positions keep their labels (train.py:259-266)."""
    rng = np.random.default_rng(31)
    text = lambda n: rng.integers(3, 92000, n)
    pre = text(20)
    pre[[3, 7, 11, 15]] = REPEATED_ID
    pre[[5, 12]] = 0
    user = text(6)
    user[2] = REPEATED_ID
    answer = text(12)
    answer[[1, 4, 6, 9]] = REPEATED_ID
    answer[10] = 0
    ids = np.concatenate([[1], pre, [92544], np.full(1024, IMG_CONTEXT), [92545], user, [92543, 525, 11353], answer, [92542],
                          np.full(12, PAD_FILL_ID)]).astype(np.int64)[None]
    assert ids.shape == (1, 1081) and not (ids == ABSENT_ID).any() and int((ids == REPEATED_ID).sum()) == 9
    amask = np.ones_like(ids)
    amask[:, -12:] = 0
    labels = ids.copy()
    a0 = int(np.nonzero((ids[0, :-2] == 92543) & (ids[0, 1:-1] == 525) & (ids[0, 2:] == 11353))[0][0])
    labels[:, :a0] = -100
    return ids, amask, labels


def _reference_trainers():
    from transformers import AutoTokenizer, GenerationConfig, get_cosine_schedule_with_warmup, AutoModel, AutoConfig  # noqa: F401
    for name in ("torchvision", "torchvision.transforms", "wandb", "PIL", "PIL.Image"):
        if name not in sys.modules:
            try:
                __import__(name)
            except Exception:
                sys.modules[name] = types.ModuleType(name)
    import train_joint_v2 as TJ
    return TJ


def _composite(real_dims: bool):
    from modeling.configuration_internvl_chat import InternVLChatConfig
    from modeling.modeling_internvl_sam import InternVLSAMModel
    sam = _sam_small(depth=2, embed_dim=768, heads=12, glob=(1,)) if real_dims else _sam_small()
    cfg = InternVLChatConfig(vision_config={"architectures": ["SAM-ViT-B-16"]}, llm_config=dict(LLM_7B_L1) if real_dims else dict(LLM_TINY),
                             downsample_ratio=0.5, template="internlm2-chat", ps_version="v2", force_image_size=1024)
    cfg.llm_config.rope_scaling = None
    m = InternVLSAMModel(cfg, vision_model=sam.image_encoder, prompt_encoder=sam.prompt_encoder, mask_decoder=sam.mask_decoder)
    if real_dims:
        fill_module_inplace(m, seed=0)
    else:
        fill_module(m, seed=0)
    return m


def _grads(m, out):
    names, none = [], []
    for name, p_ in m.named_parameters():
        if not p_.requires_grad:
            continue
        if p_.grad is None:
            none.append(name)
            continue
        g = p_.grad.numpy().reshape(-1)
        stride = max(1, g.size // 512)
        names.append(name)
        out["g:" + name] = g[::stride].copy()
        out["n:" + name] = np.float32(np.sqrt((g.astype(np.float64) ** 2).sum()))
    out["names"] = np.array(names)
    out["no_grad_names"] = np.array(none)
    return out


def case_sft(real_dims: bool = False):
    """train.py:284-318 with accumulation_steps = 1: model.train(); outputs = model(pixel_values, input_ids, attention_mask, image_flags, labels,
    return_dict=True, use_cache=False); outputs.loss.backward().  Trainable: everything but vision_model (--freeze_vision, setup_model_params
    train.py:400-480).  Stored: the loss, every gradient's sample and norm, the named rows of tok_embeddings' gradient in full, and the names of
    the trainable parameters the step leaves without a gradient."""
    m = _composite(real_dims)
    m.train()
    for n_, p_ in m.named_parameters():
        p_.requires_grad_(not n_.startswith("vision_model."))
    ids, amask, labels = sft_ids()
    x = torch.from_numpy(rand_image((1, 3, 1024, 1024), seed=32))
    tids = torch.from_numpy(ids)
    t = time.time()
    with torch.enable_grad():
        outputs = m(pixel_values=x, input_ids=tids, attention_mask=torch.from_numpy(amask), image_flags=(tids == IMG_CONTEXT)[..., None].long(),
                    labels=torch.from_numpy(labels), return_dict=True, use_cache=False, output_hidden_states=None)
        loss = outputs.loss / 1
        loss.backward()
    print(f"  reference SFT step {time.time() - t:.1f}s, loss {loss.item():.6f}")
    out = {"image_seed": 32, "ids": ids, "attention_mask": amask, "labels": labels, "loss": np.float32(loss.item()),
           "row_ids": np.array(STORED_ROWS, np.int64)}
    gt = m.language_model.model.tok_embeddings.weight.grad.numpy()
    out["emb_rows"] = gt[list(STORED_ROWS)].copy()
    save("train_sft_step_real" if real_dims else "train_sft_step", **_grads(m, out))


def case_train_step_llm():
    """train_joint_v2.py:943-1100 on the tiny composite (case_train_step's step) with --trainable_modules vision_model mlp1 language_model mlp2 prompt_encoder
    mask_decoder: model(..., labels=labels, output_hidden_states=True), the second vision_model call, prompt encoder, mask decoder, upsample, calc_instance_loss,
    loss = 0 * outputs.loss + seg_loss (:1096).  The LLM's gradients come from the segmentation loss alone; the LM head's is a tensor of zeros."""
    TJ = _reference_trainers()
    m = _composite(False)
    m.train()
    for p_ in m.parameters():
        p_.requires_grad_(True)
    x = torch.from_numpy(rand_image((1, 3, 1024, 1024), seed=14))
    ids = O.make_input_ids(n_text_pre=20, n_text_post=34, seed=1)
    tids = torch.from_numpy(ids)
    labels = ids.copy()
    labels[:, :1050] = -100
    pts = np.array([[[300.0, 340.0], [120.0, 800.0]], [[700.0, 610.0], [64.0, 64.0]]], np.float32)
    lbl = np.array([[1, 0], [1, 1]], np.int32)
    yy, xx = np.mgrid[0:1024, 0:1024].astype(np.float32)
    gt = np.stack([((xx - 300) ** 2 + (yy - 340) ** 2 < 150 ** 2), ((xx - 700) ** 2 + (yy - 610) ** 2 < 220 ** 2)]).astype(np.float32)[:, None]
    with torch.enable_grad():
        outputs = m(pixel_values=x, input_ids=tids, attention_mask=torch.ones_like(tids), image_flags=(tids == IMG_CONTEXT)[..., None].long(),
                    labels=torch.from_numpy(labels), return_dict=True, use_cache=False, output_hidden_states=True)
        image_embeddings = m.vision_model(x)
        last = outputs.hidden_states.repeat(pts.shape[0], 1, 1, 1)
        sp, de = m.prompt_encoder(points=(torch.from_numpy(pts), torch.from_numpy(lbl)), boxes=None, masks=None, llm_hidden_states=last)
        low, iou = m.mask_decoder(image_embeddings=image_embeddings, image_pe=m.prompt_encoder.get_dense_pe(),
                                  sparse_prompt_embeddings=sp, dense_prompt_embeddings=de, multimask_output=False)
        pred = torch.nn.functional.interpolate(low, (1024, 1024), mode="bilinear", align_corners=False)
        seg_loss, bce, dice, iou_val = TJ.calc_instance_loss(pred, torch.from_numpy(gt), TJ.BCELoss(), TJ.DiceLoss())
        loss = 0 * outputs.loss + seg_loss
        loss.backward()
    hg = m.language_model.output.weight.grad
    assert hg is not None and float(hg.abs().max()) == 0.0
    out = {"seed": 14, "ids": ids, "labels": labels, "pts": pts, "lbl": lbl, "loss": np.float32(loss.item()), "lm_loss": np.float32(outputs.loss.item()),
           "row_ids": np.array(STORED_ROWS, np.int64)}
    out["emb_rows"] = m.language_model.model.tok_embeddings.weight.grad.numpy()[list(STORED_ROWS)].copy()
    save("train_step_llm", **_grads(m, out))


def _one_thread(fn):
    """The relative-position tables' gradients (an indexed accumulate on the CPU) differ in their last bits from run to run on several threads."""
    def run():
        n = torch.get_num_threads()
        torch.set_num_threads(1)
        try:
            fn()
        finally:
            torch.set_num_threads(n)
    return run


CASES = {"train_sft_step": case_sft, "train_step_llm": _one_thread(case_train_step_llm), "train_sft_step_real": lambda: case_sft(real_dims=True)}

if __name__ == "__main__":
    for n in (sys.argv[1:] or list(CASES)):
        print(f"[gen_golden_train_llm] {n}")
        t0 = time.time()
        CASES[n]()
        print(f"  done in {time.time() - t0:.1f}s")
