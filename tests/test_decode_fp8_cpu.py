"""CPU-only checks of the weight-only fp8 decode (InternLM2ForCausalLM.fp8_decode): the switch and its default, the ABI (header, binding and built
library agree on version 14 and on the new entries), the quantiser's scale rule restated with torch's float8_e4m3fn (what tests/test_decode_fp8_gpu.py
holds the kernel to), the no-spill gate of the new kernels, and that the switch changes nothing where the feature does not apply (CPU tensors)."""
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("ullsam_rows_fp8_pow2", "ullsam_gemm_w8", "ullsam_decode_qkv_rope_w8")


def quant_ref(w: torch.Tensor):
    """The quantiser's definition on the CPU: per row the smallest power of two `scale` with amax / scale <= 448 (never below 2^-126; 1 for a zero row),
    then saturating round-to-nearest-even to OCP e4m3 (torch.float8_e4m3fn).  -> (uint8 bytes [N, K], fp32 scales [N])."""
    wf = w.detach().float().cpu()
    amax = wf.abs().amax(1)
    f, e = torch.frexp(amax)                       # amax = f * 2^e, f in [0.5, 1); 448 = 0.875 * 2^9
    s = torch.where(f <= 0.875, e - 9, e - 8).clamp_min(-126)
    scale = torch.where(amax > 0, torch.ldexp(torch.ones_like(amax), s), torch.ones_like(amax))
    q = (wf / scale[:, None]).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
    return q.view(torch.uint8), scale


def dequant_ref(q: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    return q.cpu().view(torch.float8_e4m3fn).float() * scale.cpu()[:, None]


def _tiny_lm(dtype=torch.float32):
    from ullsam_amd.modeling.configuration_internlm2 import InternLM2Config
    from ullsam_amd.modeling.modeling_internlm2 import InternLM2ForCausalLM
    cfg = InternLM2Config(vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=1,
                          bias=False, max_position_embeddings=2048, rope_theta=10000.0, rms_norm_eps=1e-5)
    return InternLM2ForCausalLM(cfg).to(dtype).eval()


def test_switch_defaults_to_off_and_lives_outside_the_state_dict():
    lm = _tiny_lm()
    assert lm.fp8_decode is False and lm.model.fp8_decode is False
    keys = set(lm.state_dict())
    lm.fp8_decode = True
    assert lm.fp8_decode is True and lm.model.fp8_decode is True      # the token loop calls the layer stack on its own: the stack sees the switch
    assert set(lm.state_dict()) == keys
    del lm.fp8_decode                                                 # a model without the attribute is a model with the switch off
    assert lm.fp8_decode is False and "fp8_decode" not in lm.model.__dict__
    lm.fp8_decode = False


def test_internvl_sam_reaches_the_switch_through_language_model():
    src = open(os.path.join(ROOT, "ullsam_amd", "modeling", "modeling_internvl_sam.py")).read()
    assert "self.language_model" in src
    from ullsam_amd.modeling.modeling_internlm2 import InternLM2ForCausalLM
    assert isinstance(InternLM2ForCausalLM.fp8_decode, property)


def test_header_binding_and_library_agree_on_version_14_and_the_new_entries():
    from ullsam_amd import build, _lib
    hdr = open(os.path.join(ROOT, "include", "ullsam_hip.h")).read()
    assert int(re.search(r"#define ULLSAM_ABI_VERSION (\d+)", hdr).group(1)) == 14 == _lib.ABI_VERSION
    decl = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    build.build(verbose=False)
    lib = _lib.load()
    assert lib.ullsam_abi_version() == 14
    for name in NEW_ENTRIES:
        m = re.search(r"\b" + name + r"\s*\(([^;]*)\)\s*;", decl)
        assert m, f"{name} not declared in include/ullsam_hip.h"
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name]), name     # one ctypes entry per declared argument
        assert hasattr(lib, name), f"{name} not exported by the built library"
    # the reference lines the entries stand for are cited, as the header's custom is
    assert "modeling_internlm2.py:261-264, 341-426, 1081-1082" in hdr


def test_scale_rule_restated_with_torch_float8():
    """The definition itself, where it can be checked without a GPU: power-of-two scales, the smallest that fits, q * scale exact in bf16, a fixed point."""
    g = torch.Generator().manual_seed(3)
    w = (torch.randn(64, 1024, generator=g) * 0.02).to(torch.bfloat16)
    w[0] = 0
    w[1, 5] = 448.0 * 2.0 ** -3          # amax an exact power of two times 448: the scale 2^-3 fits exactly, code 448
    w[2, 7] = 1000.0                     # one outlier
    q, sc = quant_ref(w)
    f, _ = torch.frexp(sc)
    assert bool((f == 0.5).all()) and float(sc[0]) == 1.0 and float(sc[1]) == 2.0 ** -3 and int(q[1, 5]) == 0x7E
    amax = w.float().abs().amax(1)
    nz = amax > 0
    assert bool((amax[nz] / sc[nz] <= 448).all()) and bool((amax[nz] / (sc[nz] / 2) > 448).all())
    wd = dequant_ref(q, sc)
    assert torch.equal(wd.to(torch.bfloat16).float(), wd)
    q2, sc2 = quant_ref(wd.to(torch.bfloat16))
    assert torch.equal(dequant_ref(q2, sc2), wd)
    rel = float((wd - w.float())[3:].pow(2).mean().sqrt() / w.float()[3:].pow(2).mean().sqrt())
    assert rel < 0.04, rel               # e4m3: 3 mantissa bits, relative rms error ~ 2^-4 / sqrt(3) at worst, ~0.027 on gaussian rows


def test_decode_w8_ok_names_the_shapes_the_bf16_decode_kernels_take():
    from ullsam_amd import ops
    assert ops.decode_w8_ok(4, 4096) and ops.decode_w8_ok(1, 14336) and ops.decode_w8_ok(8, 1536) and ops.decode_w8_ok(4, 512)
    assert not ops.decode_w8_ok(9, 4096) and not ops.decode_w8_ok(0, 4096) and not ops.decode_w8_ok(4, 1000) and not ops.decode_w8_ok(4, 20480)
    assert not ops.decode_w8_ok(8, 14336)     # 8 rows x 14336 bf16 do not fit the LDS: the bf16 GEMM leaves the decode kernels there too


def test_new_kernels_compile_without_spills():
    from ullsam_amd import build
    build.build(verbose=False)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    ks = KR.kernels()
    new = {n: r for n, r in ks.items() if any(re.search(h, n) for h in KR.HOT_DECODE_FP8)}
    for must in ("rows_fp8_pow2_kernel", "gemm_skinny_kernel", "gemm_skinny_persist_kernel", "gemm_skinny_ksplit_kernel"):
        assert any(must + "I" in n for n in new), (must, sorted(new))
    assert len(new) == 10, sorted(new)        # 2 quantisers + 3 + 2 + 3 e4m3-weight GEMM forms
    bad = {n: r for n, r in new.items() if r.get("vgpr_spill_count", 0) or r.get("sgpr_spill_count", 0) or r.get("private_segment_fixed_size", 0)}
    assert not bad, bad
    # half the weight dwords per register buffer: no e4m3 form may need more registers than its bf16 twin
    for n, r in new.items():
        twin = ks.get(n.replace("Lb1EEv8GemmArgs", "Lb0EEv8GemmArgs"))
        if twin is not None and "GemmArgs" in n:
            assert r["vgpr_count"] <= twin["vgpr_count"], (n, r["vgpr_count"], twin["vgpr_count"])


def test_cpu_tensors_behave_as_before_with_the_switch_on(monkeypatch):
    """There is no CPU path, with or without the switch: the same error from the same place, and no e4m3 entry is reached."""
    from ullsam_amd import _lib
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: calls.append(name))
    lm = _tiny_lm()
    ids = torch.randint(0, 512, (1, 5))
    msgs = []
    for on in (False, True):
        lm.fp8_decode = on
        with pytest.raises(_lib.UllsamError) as ei:
            lm.generate(input_ids=ids, max_new_tokens=2, eos_token_id=-1)
        msgs.append(str(ei.value))
    assert msgs[0] == msgs[1] and "GPU" in msgs[0]
    assert not any("w8" in c or "fp8" in c for c in calls), calls


def test_prepack_takes_the_keyword():
    import inspect
    from ullsam_amd import checkpoint
    sig = inspect.signature(checkpoint.prepack)
    assert sig.parameters["fp8_decode"].default is False and sig.parameters["fp8_vit"].default is False
    assert checkpoint.prepack(_tiny_lm(), fp8_decode=True) == checkpoint.prepack(_tiny_lm())     # a CPU / fp32 model: nothing to quantise, nothing attempted
