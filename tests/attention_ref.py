"""Float64 definitions of the two prefill attention entry points (ullsam_causal_attention, ullsam_vit_attention), probe values that make a
kernel hand out its probability matrix, a model of what the bf16 format alone costs, and the case tables that tests/test_attention_ref_cpu.py
checks and tests/test_attention_kernels_gpu.py runs.  Plain torch, no GPU needed: every function works on the device of its operands.

Why probabilities and not outputs: with random V over hundreds of keys an output is a mean of about 1 / sqrt(keys), and an absolute bound on it
hides a dropped key block, a rel-pos term on the wrong key or a masked key with weight.  With V one-hot (probe_v) the output IS a slice of the
probability matrix, and every entry is compared relative to itself."""
import math
import zlib

import torch

FMIN = float(torch.finfo(torch.float32).min)
BF16_TOL = 2.0 ** -6          # per entry, relative: three half-ulps of bf16 for the format (bf16_model) and one for fp32 arithmetic and v_exp_f32
FORMAT_TOL = 3 * 2.0 ** -8    # what bf16_model may cost: P, the denominator summed from rounded P, the output
P_FLOOR = 2.0 ** -100         # absolute term of the bound; the tables keep every compared probability >= MIN_P so that it never decides
MIN_P = 2.0 ** -90
MAX_LOGIT = 2.0 ** 7
MAX_SPAN = 48.0               # nats between the largest and smallest unmasked logit of a row
MAX_RUNS = 16                 # probe launches per case
F32_MARGIN = 4.0              # the fp32 kernels get 4 x the error of a plain float32 evaluation of the same definition (summation order, online
                              # rescaling, hardware exponential)


def _gen(name):
    g = torch.Generator()
    g.manual_seed(zlib.crc32(name.encode()))
    return g


# ---------------------------------------------------------------------------------------------------------------- causal
def causal_ref(q, k, v, key_mask, q_pos0, dtype=torch.float64):
    """q [B, Sq, H, hd], k / v [B, KVH, Sk, hd], key_mask [B, Sk] (1 = attend) or None -> (out [B, Sq, H, hd], P [B, H, Sq, Sk], defined [B, Sq]).
    The reference's additive masks, literally (modeling_internlm2.py:96-125,830-851): finfo(float32).min for a future key plus finfo.min for a
    padded key, summed and added to the scaled score in float32 -- one mask absorbs the score, two give -inf -- then softmax in `dtype`.
    A row is defined when it sees at least one unmasked key; there every masked key has probability exactly 0.  The other rows (left-padded
    queries) come out as the reference's uniform rows and are not what the kernels promise (finite, a convex combination of V rows).
    dtype=float32 is the plain single-precision evaluation that the fp32 kernels' bound is measured from."""
    B, Sq, H, hd = q.shape
    KVH, Sk = k.shape[1], k.shape[2]
    G = H // KVH
    qf = q.to(dtype).permute(0, 2, 1, 3)
    kf = k.to(dtype).repeat_interleave(G, 1)
    vf = v.to(dtype).repeat_interleave(G, 1)
    sc = qf @ kf.transpose(-1, -2) / math.sqrt(hd)
    dev = q.device
    qpos = q_pos0 + torch.arange(Sq, device=dev)[:, None]
    future = torch.arange(Sk, device=dev)[None, :] > qpos                                   # [Sq, Sk]
    padded = torch.zeros(B, 1, Sk, dtype=torch.bool, device=dev) if key_mask is None else (key_mask == 0)[:, None, :]
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    add = torch.where(future, FMIN, zero)[None] + torch.where(padded, FMIN, zero)           # float32: finfo.min + finfo.min = -inf
    add = add[:, None]                                                                      # [B, 1, Sq, Sk]
    x = torch.where(add == 0, sc, (sc.float() + add).to(dtype))                             # unmasked scores keep their precision
    m = x.max(-1, keepdim=True).values
    e = torch.exp(x - m)
    P = e / e.sum(-1, keepdim=True)
    out = (P @ vf).permute(0, 2, 1, 3)
    defined = (~(future[None] | padded)).any(-1)
    return out, P, defined


def causal_unmasked(key_mask, B, Sq, Sk, q_pos0, device="cpu"):
    """[B, Sq, Sk] True where the key is neither in the future nor padded."""
    qpos = q_pos0 + torch.arange(Sq, device=device)[:, None]
    ok = (torch.arange(Sk, device=device)[None, :] <= qpos)[None].expand(B, Sq, Sk)
    return ok if key_mask is None else ok & (key_mask != 0)[:, None, :]


# ---------------------------------------------------------------------------------------------------------------- ViT
def window_layout(gh, gw, window):
    """-> (tok [nwin, W*W] token index in the gh x gw grid, -1 for a pad token; nh, nw)."""
    nh, nw = -(-gh // window), -(-gw // window)
    y = torch.arange(nh * window)[:, None].expand(nh * window, nw * window)
    x = torch.arange(nw * window)[None, :].expand(nh * window, nw * window)
    tok = torch.where((y < gh) & (x < gw), y * gw + x, -1)
    tok = tok.reshape(nh, window, nw, window).permute(0, 2, 1, 3).reshape(nh * nw, window * window)
    return tok, nh, nw


def vit_logits(qkv, rel_h, rel_w, qkv_bias, B, heads, hd, gh, gw, window, dtype=torch.float64, parent_indexing=False):
    """-> (logits [B, nwin, heads, N, N], v [B, nwin, heads, N, hd], tok [nwin, N]); nwin = 1 and N = gh*gw for window == 0.
    parent_indexing: what flash_attn_kernel's global table pass computed before it sized each table by its own side -- the rel_h row
    q - k + (gw - 1) out of 2*gw - 1 staged rows; a row past the 2*gh - 1 that exist (beyond the allocation on the GPU) or a slot that
    was never written counts as 0 here, the kindest value it could have had."""
    dev = qkv.device
    D = heads * hd
    t = qkv.to(dtype).reshape(B, gh * gw, 3, heads, hd)
    if window > 0:
        tok, nh, nw = window_layout(gh, gw, window)
        tok = tok.to(dev)
        pad = qkv_bias.to(dtype).reshape(1, 1, 3, heads, hd)
        full = torch.cat([t, pad.expand(B, 1, 3, heads, hd)], 1)                            # token -1 = the pad token: q = k = v = qkv.bias
        win = full[:, tok]                                                                  # [B, nwin, N, 3, heads, hd]
        Gh = Gw = window
    else:
        tok = torch.arange(gh * gw, device=dev)[None]
        win = t[:, None]
        Gh, Gw = gh, gw
    win = win.permute(0, 1, 3, 4, 2, 5)                                                     # [B, nwin, 3, heads, N, hd]
    q, k, v = win[:, :, 0], win[:, :, 1], win[:, :, 2]
    assert rel_h.shape == (2 * Gh - 1, hd) and rel_w.shape == (2 * Gw - 1, hd), "tables are per side"
    ih = torch.arange(Gh, device=dev)
    iw = torch.arange(Gw, device=dev)
    Rw = rel_w.to(dtype)[iw[:, None] - iw[None, :] + Gw - 1]                                # [qw, kw, hd]
    if parent_indexing and window == 0:
        e = ih[:, None] - ih[None, :] + Gw - 1
        ok = (e >= 0) & (e < 2 * Gw - 1) & (e < 2 * Gh - 1)
        Rh = rel_h.to(dtype)[e.clamp(0, 2 * Gh - 2)] * ok[:, :, None]
    else:
        Rh = rel_h.to(dtype)[ih[:, None] - ih[None, :] + Gh - 1]                            # [qh, kh, hd]
    qg = q.reshape(B, -1, heads, Gh, Gw, hd)                                                # the UNSCALED q (image_encoder.py:231-234)
    bh = torch.einsum("bnahwc,hkc->bnahwk", qg, Rh)
    bw = torch.einsum("bnahwc,wkc->bnahwk", qg, Rw)
    N = Gh * Gw
    bias = (bh[..., :, None] + bw[..., None, :]).reshape(B, -1, heads, N, N)
    logits = q @ k.transpose(-1, -2) * (hd ** -0.5) + bias
    return logits, v, tok


def vit_ref(qkv, rel_h, rel_w, qkv_bias, B, heads, hd, gh, gw, window, dtype=torch.float64, parent_indexing=False):
    """The packed operands as the kernel sees them -> (out [B*gh*gw, heads*hd], P [B, nwin, heads, N, N]).  Decomposed rel-pos bias from the
    unscaled q; pad tokens of partial windows have q = k = v = qkv.bias and are live keys, their query rows are cropped; tables per side
    (2*gh-1 and 2*gw-1 rows, 2*window-1 for both in window mode)."""
    logits, v, tok = vit_logits(qkv, rel_h, rel_w, qkv_bias, B, heads, hd, gh, gw, window, dtype, parent_indexing)
    P = torch.softmax(logits, -1)
    o = (P @ v).permute(0, 1, 3, 2, 4)                                                      # [B, nwin, N, heads, hd]
    out = torch.zeros(B, gh * gw, heads, hd, dtype=dtype, device=qkv.device)
    live = tok >= 0
    out[:, tok[live]] = o[:, live]
    return out.reshape(B * gh * gw, heads * hd), P


def vit_token_p(P, tok, gh, gw):
    """P [B, nwin, heads, N, N] -> [B, gh*gw, heads, N + 1] in the layout of the kernel's output rows: per live query token its window's
    probabilities by local key index, the pad keys' entries moved into ONE extra slot (their sum).  Every pad key's V is the same vector
    (qkv.bias), so no probe can tell two of them apart: their total is what a kernel can be asked for."""
    B, nwin, heads, N, _ = P.shape
    live = tok >= 0                                                                         # [nwin, N]
    Pl = P * live[None, :, None, None, :]
    agg = (P * (~live)[None, :, None, None, :]).sum(-1, keepdim=True)
    full = torch.cat([Pl, agg], -1).permute(0, 1, 3, 2, 4)                                  # [B, nwin, N(query), heads, N + 1]
    out = torch.zeros(B, gh * gw, heads, N + 1, dtype=P.dtype, device=P.device)
    out[:, tok[live]] = full[:, live]
    return out


def vit_token_keys(tok, gh, gw):
    """[gh*gw, N + 1] True where the slot of vit_token_p holds a probability to compare (a live key, or the pad slot of a window with pads)."""
    nwin, N = tok.shape
    live = tok >= 0
    slots = torch.cat([live, (~live).any(-1, keepdim=True)], -1)                            # [nwin, N + 1]
    out = torch.zeros(gh * gw, N + 1, dtype=torch.bool, device=tok.device)
    out[tok[live]] = slots[:, None, :].expand(nwin, N, N + 1)[live]
    return out


# ---------------------------------------------------------------------------------------------------------------- probes
def probe_v(n_keys, hd, run, dtype=torch.float32):
    """V [n_keys, hd], one-hot at column k - run*hd for the keys of [run*hd, (run+1)*hd), zero elsewhere: the kernel's output columns are then
    columns run*hd ... of its probability matrix.  ceil(n_keys / hd) launches return every entry."""
    v = torch.zeros(n_keys, hd, dtype=dtype)
    ks = torch.arange(run * hd, min((run + 1) * hd, n_keys))
    v[ks, ks - run * hd] = 1
    return v


def n_runs(n_keys, hd):
    return -(-n_keys // hd)


def recover_p(outputs, n_keys):
    """outputs[run] [..., hd] -> [..., n_keys]"""
    return torch.cat(list(outputs), -1)[..., :n_keys]


# ---------------------------------------------------------------------------------------------------------------- rounding model
def bf16_model(logits):
    """What the bf16 format alone costs, on the CPU: float32 exponentials rounded to bf16 (the P operand of the PV product), a denominator from
    the unrounded sum or from the rounded sum (the kernels that take it out of the PV product through a column of ones: LSUM_MFMA, win14,
    vitglob), the quotient rounded to bf16 (the stored output).  logits [..., N], -inf = masked.  -> (P from the unrounded sum, P from the rounded sum)."""
    x = logits.float()
    e = torch.exp(x - x.max(-1, keepdim=True).values)
    eb = e.bfloat16().float()
    return tuple((eb / d.sum(-1, keepdim=True)).bfloat16().double() for d in (e, eb))


def rel_err(got, ref, keep):
    """Largest |got - ref| / ref over the entries of `keep`."""
    return float(((got.double() - ref).abs() / ref.clamp_min(1e-300))[keep].max()) if bool(keep.any()) else 0.0


# ---------------------------------------------------------------------------------------------------------------- the two checks
def check_entries(got, ref, keep, tol, what):
    """|got - ref| <= tol * ref + 2^-100 on the entries of keep; -> the largest relative error (printed before it is asserted)."""
    err = (got.double() - ref).abs()
    worst = float((err / ref.clamp_min(1e-300))[keep].max())
    print(f"{what}: probabilities, largest relative error {worst:.3e} (bound {tol:.3e}) over {int(keep.sum())} entries")
    bad = (err > tol * ref + P_FLOOR) & keep
    assert not bool(bad.any()), (what, worst, tol, int(bad.sum()), bad.nonzero()[:4].tolist())
    return worst


def check_outputs(got, ref, rows, tol, what):
    """got / ref [..., hd], rows [...]: error normalised per row by the row's largest reference output."""
    scale = ref.abs().max(-1, keepdim=True).values
    rel = ((got.double() - ref).abs() / scale.clamp_min(1e-300))[rows]
    worst = float(rel.max())
    print(f"{what}: random V, largest row-normalised output error {worst:.3e} (bound {tol:.3e})")
    assert worst <= tol, (what, worst, tol)
    return worst


# ---------------------------------------------------------------------------------------------------------------- causal cases
# name -> what differs from B 2, H 4, KVH 2, random logits, cap = Sk + 5.  mask: batch row 0 always sees every key, the LAST batch row gets
# ("left", n) | ("holes", [..]) | ("range", a, b) | ("tail", n); absent -> left padding of min(3, Sk - 1) keys; None -> no mask operand at all.
def _c(Sq, q_pos0, **kw):
    return dict(Sq=Sq, q_pos0=q_pos0, **kw)


CAUSAL_SHAPES = {f"sq{a}_past{b}": _c(a, b) for a, b in
                 [(2, 0), (31, 0), (32, 0), (33, 0), (64, 0), (65, 0), (127, 0), (128, 0), (129, 0), (257, 0),
                  (1, 63), (1, 64), (2, 126), (5, 123), (33, 31), (64, 64), (96, 65), (130, 62), (200, 190)]}
CAUSAL_LEFTPAD = {**{f"sq200_left{n}": _c(200, 0, mask=("left", n)) for n in (1, 31, 32, 33, 63, 64, 65, 128, 129)},
                  **{f"sq130_past62_left{n}": _c(130, 62, mask=("left", n)) for n in (40, 62, 63, 100)}}
CAUSAL_MASKS = {"hole40": _c(200, 0, mask=("holes", [40])), "hole_tile_64_127": _c(200, 0, mask=("range", 64, 128)),
                "holes_0_33_199": _c(200, 0, mask=("holes", [0, 33, 199])), "tail70": _c(200, 0, mask=("tail", 70))}
CAUSAL_GQA = {f"gqa_h{h}_kvh{k}": _c(70, 0, H=h, KVH=k, mask=None if i % 2 == 0 else ("left", 5))
              for i, (h, k) in enumerate([(1, 1), (2, 1), (4, 4), (8, 1), (6, 2)])}
CAUSAL_LOGITS = {f"logits_{n}": _c(200, 0, logits=n) for n in ("rand1", "rand4", "rising", "falling", "spike_key0", "spike_diag")}
CAUSAL_FAMILIES = {"shapes": CAUSAL_SHAPES, "leftpad": CAUSAL_LEFTPAD, "masks": CAUSAL_MASKS, "gqa": CAUSAL_GQA, "logits": CAUSAL_LOGITS}
# kernel name -> (dtype, head_dim, ullsam_set_attn_variant)
CAUSAL_KERNELS = {"causal128": (torch.bfloat16, 128, 0), "tiled_v11": (torch.bfloat16, 128, 11), "fp32": (torch.float32, 128, 0),
                  "hd64_bf16": (torch.bfloat16, 64, 0), "hd64_fp32": (torch.float32, 64, 0)}
RAMP_STEP = 0.2               # nats per key: 199 steps = 39.8 nats, inside MAX_SPAN


def causal_mask(c, B, Sk):
    m = c.get("mask", ("left", min(3, Sk - 1)))
    if m is None:
        return None
    M = torch.ones(B, Sk, dtype=torch.int32)
    if m[0] == "left":
        M[-1, :m[1]] = 0
    elif m[0] == "holes":
        M[-1, m[1]] = 0
    elif m[0] == "range":
        M[-1, m[1]:m[2]] = 0
    elif m[0] == "tail":
        M[-1, Sk - m[1]:] = 0
    return M


def build_causal(name, c, dtype, hd):
    """-> dict(q [B, Sq, H, hd], k, v [B, KVH, Sk, hd] in `dtype` (the reference reads the rounded values), mask int32 [B, Sk] | None, ...)."""
    B, H, KVH, Sq, p0 = c.get("B", 2), c.get("H", 4), c.get("KVH", 2), c["Sq"], c["q_pos0"]
    Sk = p0 + Sq
    g = _gen(f"causal/{name}/{hd}")
    q = torch.randn(B, Sq, H, hd, generator=g)
    k = torch.randn(B, KVH, Sk, hd, generator=g)
    v = torch.randn(B, KVH, Sk, hd, generator=g)
    kind = c.get("logits", "rand1")
    u = torch.where(torch.rand(hd, generator=g) < 0.5, -1.0, 1.0)                           # |u|^2 = hd: (s u) . (c u) / sqrt(hd) = s c sqrt(hd)
    if kind == "rand4":
        q = q * 4
    elif kind in ("rising", "falling"):                                                     # k_j = c_j u, q = s u: score = s c_j sqrt(hd), a ramp along the keys
        cj = torch.arange(Sk) * (RAMP_STEP / math.sqrt(hd)) * (1 if kind == "rising" else -1)
        k = (cj[:, None] * u).expand(B, KVH, Sk, hd).clone()
        s = 1 - 0.1 * torch.arange(H) / H
        q = (s[:, None] * u).expand(B, Sq, H, hd).clone()
    elif kind == "spike_key0":                                                              # key 0 about 20 nats above the rest, for every query
        q = q + u
        k[:, :, 0] = u * (20 / math.sqrt(hd))
    elif kind == "spike_diag":                                                              # the query's own key about 17 nats above the rest
        q = 0.5 * q + 1.5 * k[:, :, p0:].repeat_interleave(H // KVH, 1).permute(0, 2, 1, 3)
    return dict(q=q.to(dtype), k=k.to(dtype), v=v.to(dtype), mask=causal_mask(c, B, Sk), B=B, H=H, KVH=KVH, hd=hd, Sq=Sq, Sk=Sk, q_pos0=p0,
                cap=Sk + c.get("cap_extra", 5))


# ---------------------------------------------------------------------------------------------------------------- ViT cases
def _v(gh, gw, window, hd, B, heads, logits="rand"):
    return dict(gh=gh, gw=gw, window=window, hd=hd, B=B, heads=heads, logits=logits)


WINDOW14_CASES = {**{f"win14_{a}x{b}": _v(a, b, 14, 80, 2, 3) for a, b in [(14, 14), (15, 15), (28, 28), (29, 29), (16, 30), (30, 16), (57, 14)]},
                  "win14_64x64": _v(64, 64, 14, 80, 1, 1),
                  **{f"win14_29x29_{n}": _v(29, 29, 14, 80, 2, 3, n) for n in ("q6", "rel", "bias")}}
# kernel name -> (dtype, variant)
WINDOW14_KERNELS = {"win14r": (torch.bfloat16, 0), "win14_v13": (torch.bfloat16, 13), "tiled4_v2": (torch.bfloat16, 2), "tiled7_v1": (torch.bfloat16, 1),
                    "fp32": (torch.float32, 0)}
WINDOW_OTHER_CASES = {"win7_10x10": _v(10, 10, 7, 64, 2, 3), "win8_9x17": _v(9, 17, 8, 64, 2, 3), "win13_14x14": _v(14, 14, 13, 80, 2, 3)}
WINDOW_OTHER_KERNELS = {"tiled4": (torch.bfloat16, 0), "tiled7_v1": (torch.bfloat16, 1), "fp32": (torch.float32, 0)}
GLOBAL_SMALL_GRIDS = [(1, 1), (2, 2), (7, 7), (8, 8), (8, 9), (33, 33)]
GLOBAL_NONSQUARE_GRIDS = [(5, 64), (64, 5), (33, 20)]                                       # not before the table pass sizes rel_h by grid_h
GLOBAL_SMALL_CASES = {f"glob_{a}x{b}_hd{hd}": _v(a, b, 0, hd, 2 if a * b < 1000 else 1, 2)
                      for a, b in GLOBAL_SMALL_GRIDS + GLOBAL_NONSQUARE_GRIDS for hd in (64, 80)
                      if (a * b, hd) != (1089, 64)}                                         # 33 x 33 at hd 64 would take 18 probe launches; at hd 80 it takes 14
GLOBAL_SMALL_KERNELS = {"bf16": (torch.bfloat16, 0), "fp32": (torch.float32, 0)}
GLOBAL64_CASES = {"glob_64x64_hd80": _v(64, 64, 0, 80, 1, 2), "glob_64x64_hd64": _v(64, 64, 0, 64, 1, 2)}
# kernel name -> (dtype, variant, case)
GLOBAL64_KERNELS = {"vitglob": (torch.bfloat16, 0, "glob_64x64_hd80"), "tiled8_v12": (torch.bfloat16, 12, "glob_64x64_hd80"),
                    "tiled4_v9": (torch.bfloat16, 9, "glob_64x64_hd80"), "fp32": (torch.float32, 0, "glob_64x64_hd80"),
                    "hd64_bf16": (torch.bfloat16, 0, "glob_64x64_hd64")}
VIT_FAMILIES = {"window14": WINDOW14_CASES, "window_other": WINDOW_OTHER_CASES, "global_small": GLOBAL_SMALL_CASES, "global64": GLOBAL64_CASES}


def build_vit(name, c, dtype):
    """-> dict(qkv [B*gh*gw, 3*heads*hd], rel_h, rel_w, bias [3*heads*hd]) in `dtype`."""
    gh, gw, W, hd, B, heads = c["gh"], c["gw"], c["window"], c["hd"], c["B"], c["heads"]
    D = heads * hd
    g = _gen(f"vit/{name}")
    qkv = torch.randn(B * gh * gw, 3, heads, hd, generator=g)
    nh_, nw_ = (W, W) if W > 0 else (gh, gw)
    kind = c["logits"]
    tscale = {"rand": 0.1, "q6": 0.02, "rel": 0.45, "bias": 0.1}[kind]
    rel_h = torch.randn(2 * nh_ - 1, hd, generator=g) * tscale
    rel_w = torch.randn(2 * nw_ - 1, hd, generator=g) * tscale
    bias = torch.randn(3, heads, hd, generator=g) * 0.3
    if kind == "q6":                                                                        # q scaled by 6; k by 0.8 and small tables keep a row's span <= MAX_SPAN
        qkv[:, 0] *= 6
        qkv[:, 1] *= 0.8
    elif kind == "bias":                                                                    # pad keys about sqrt(hd) nats above the live ones
        u = torch.where(torch.rand(hd, generator=g) < 0.5, -1.0, 1.0)
        qkv[:, 0] += u
        bias[0] = u
        bias[1] = u
    return dict(qkv=qkv.reshape(-1, 3 * D).to(dtype), rel_h=rel_h.to(dtype), rel_w=rel_w.to(dtype), bias=bias.reshape(3 * D).to(dtype), **c)


def vit_probe_qkv(qkv, bias, case, run, mode="keys"):
    """The operands with V replaced by probe values (q and k untouched) -> (qkv, bias).
    mode "keys": token -> one-hot of its (window-local) key index, slot N = every pad token through bias_v; run selects hd of the N + 1 slots.
    mode "row" / "col" (global only, side <= hd): one-hot of the key's grid row / column: the output is that marginal of the probability matrix."""
    gh, gw, W, hd, B, heads = case["gh"], case["gw"], case["window"], case["hd"], case["B"], case["heads"]
    D = heads * hd
    t = torch.arange(gh * gw)
    y, x = t // gw, t % gw
    if mode == "keys":
        local = (y % W) * W + (x % W) if W > 0 else t
        N = W * W if W > 0 else gh * gw
        table = probe_v(N + 1, hd, run, torch.float32)                                      # [N + 1, hd]
        vt, vpad = table[local], table[N]
    else:
        assert W == 0 and max(gh, gw) <= hd
        vt, vpad = probe_v(hd, hd, 0)[y if mode == "row" else x], torch.zeros(hd)
    q2 = qkv.clone().reshape(B, gh * gw, 3, heads, hd)
    q2[:, :, 2] = vt[None, :, None, :].to(qkv.dtype)
    b2 = bias.clone().reshape(3, heads, hd)
    b2[2] = vpad.to(bias.dtype)
    return q2.reshape(-1, 3 * D), b2.reshape(3 * D)


def vit_probe_runs(case):
    N = case["window"] ** 2 if case["window"] > 0 else case["gh"] * case["gw"]
    has_pad = case["window"] > 0 and (case["gh"] % case["window"] or case["gw"] % case["window"])
    return n_runs(N + 1 if has_pad else N, case["hd"])
