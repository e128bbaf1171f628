"""Float64 definitions of the fused mask-decoder launches (csrc/dectok.hip, csrc/decoder.hip), one function per launch, written from the reference's
TwoWayAttentionBlock / Attention (modeling/transformer.py:153-242) and MaskDecoder.predict_masks / MLP (modeling/mask_decoder.py:112-176), in plain torch
(CPU or device: everything follows the inputs' device), and the seeded inputs of tests/test_decoder_ref_cpu.py and tests/test_decoder_kernels_gpu.py.

Weights enter as their bf16-rounded values, every other input as given (fp32 or bf16); everything inside is float64.  Each definition takes a hook `r`
applied to every activation at the door of a linear (in `i2t` also to q, the scaled token keys, the probabilities and the token values entering the two
attention products):
    ident : D,  the definition;
    bf1   : D1, one bf16 term per activation -- autocast's arithmetic, the yardstick the kernels' limits are stated in;
    bf2   : D2, two bf16 terms (x = hi + lo) -- the arithmetic the kernels declare.
Declared roundings (switchable): `i2t` casts the attention output to bf16 before the output projection (the unfused path's cast to the compute dtype), `up2`
rounds the GELU of the second transposed convolution to bf16 (the upscaled embedding was a bf16 tensor between two launches)."""
import math

import torch

F64 = torch.float64
C, CI, HEADS = 256, 128, 8          # embedding, internal width of the cross attentions, heads
EPS = 1e-5                          # nn.LayerNorm default (transformer.py:133-143); LayerNorm2d uses 1e-6 (common.py)


# ---- hooks -------------------------------------------------------------------------------------------------------------------------------
def ident(x):
    return x


def _bf(x):
    return x.to(torch.float32).to(torch.bfloat16).to(F64)


def bf1(x):
    return _bf(x)


def bf2(x):
    hi = _bf(x)
    return hi + _bf(x - hi)


HOOKS = {"D": ident, "D1": bf1, "D2": bf2}


# ---- building blocks ---------------------------------------------------------------------------------------------------------------------
def _d(t):
    return None if t is None else t.to(F64)


def linear(x, W, b, r=ident):
    y = r(x) @ _d(W).T
    return y if b is None else y + _d(b)


def layer_norm(x, w, b, eps):
    mu = x.mean(-1, keepdim=True)
    d = x - mu
    y = d / torch.sqrt((d * d).mean(-1, keepdim=True) + eps)
    if w is not None:
        y = y * _d(w)
    if b is not None:
        y = y + _d(b)
    return y


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def attention_core(q, k, v, heads, scale=None):
    """softmax(q k^T / sqrt(d)) v per head, heads recombined (transformer.py:229-240); q [B, Nq, E], k / v [B, Nk, E]"""
    B, Nq, E = q.shape
    d = E // heads
    sep = lambda x: x.reshape(B, x.shape[1], heads, d).transpose(1, 2)
    s = (sep(q) @ sep(k).transpose(-1, -2)) * (1.0 / math.sqrt(d) if scale is None else scale)
    return (torch.softmax(s, -1) @ sep(v)).transpose(1, 2).reshape(B, Nq, E)


# ---- one function per launch -------------------------------------------------------------------------------------------------------------
def tok_attn(queries, qpe, Wq, bq, Wk, bk, Wv, bv, Wo, bo, ln_w, ln_b, eps, Wq2, bq2, skip_pe, mode, r=ident):
    """ullsam_dec_tok_attn.  queries / qpe [P, T, 256].  mode 0: the block's self attention (layer 0 = skip_pe: q = k = v = queries and NO residual,
    transformer.py:157-158; else q = k = queries + pe, v = queries, residual :160-162), norm1, then the q projection of the token -> image attention on
    (norm1's output + pe) (:166-167, Attention.forward :221).  mode 1: only that projection, of (queries + pe) (the final attention, transformer.py:99-100).
    -> (queries' | None in mode 1, q_t2i [P, T, 128])"""
    x, pe = _d(queries), _d(qpe)
    if mode == 1:
        return None, linear(x + pe, Wq2, bq2, r)
    qin = x if skip_pe else x + pe
    a = attention_core(linear(qin, Wq, bq, r), linear(qin, Wk, bk, r), linear(x, Wv, bv, r), HEADS)
    y = linear(a, Wo, bo, r)
    if not skip_pe:
        y = x + y
    y = layer_norm(y, ln_w, ln_b, eps)
    return y, linear(y + pe, Wq2, bq2, r)


def tok_mlp(queries, attn, qpe, Wo, bo, ln2, W1, b1, W2, b2, ln3, Wk, bk, Wv, bv, do_mlp, r=ident):
    """ullsam_dec_tok_mlp.  queries [P, T, 256] (after norm1), attn [P, T, 128] (the token -> image attention's recombined heads, before its out
    projection); ln2 / ln3 = (w, b, eps).  out projection + residual, norm2 (transformer.py:168-169); do_mlp: the MLP (lin1, ReLU, lin2) + residual,
    norm3 (:172-174), and the image -> token attention's k projection of (queries + pe) and v projection of queries (:177-178: the TOKENS are its keys).
    do_mlp 0 is the final attention with norm_final_attn (:101-104).  -> (queries', k | None, v | None)"""
    x = _d(queries) + linear(_d(attn), Wo, bo, r)
    x = layer_norm(x, *ln2)
    if not do_mlp:
        return x, None, None
    x = x + linear(torch.relu(linear(x, W1, b1, r)), W2, b2, r)
    x = layer_norm(x, *ln3)
    return x, linear(x + _d(qpe), Wk, bk, r), linear(x, Wv, bv, r)


def heads(hs, chains, m0, nm, n_iou, r=ident):
    """ullsam_dec_heads.  hs [P, T, 256]; chains = 5 lists of three (W, b): hypernetwork MLP i on mask token 1 + i (mask_decoder.py:139-142), chain 4 = the
    IoU head on token 0 (:133,147); Linear, ReLU, Linear, ReLU, Linear (:171-176).  -> (hyper [P, nm, 32] for masks m0 .. m0 + nm - 1, iou [P, n_iou])"""
    def mlp(x, layers):
        for i, (W, b) in enumerate(layers):
            x = linear(x, W, b, r)
            if i < len(layers) - 1:
                x = torch.relu(x)
        return x
    x = _d(hs)
    hyper = torch.stack([mlp(x[:, 1 + i], chains[i]) for i in range(m0, m0 + nm)], 1)
    return hyper, mlp(x[:, 0], chains[4])[:, :n_iou]


def i2t(xin, res, Wq, bq, ktok, vtok, Wo, bo, lnw, lnb, eps, key_pe, scale, r=ident, cast=True, parts=False):
    """ullsam_i2t_block: the image -> token attention of a block and norm4 (transformer.py:176-182).  xin = (keys + pe) as the bf16 tensor the image side
    carries, [P | 1, N, 256] (1: one image shared by every prompt); res = keys fp32, alike; ktok / vtok [P, T, 128] = the tokens' projected keys / values
    (tok_mlp's k, v).  q = xin Wq^T + bq; 8 heads of 16: softmax(q k^T * scale) v; the recombined heads are cast to bf16 (`cast`: the declared rounding) and
    go through the output projection; + keys; norm4.  key_pe does not enter the fp32 output (the kernel's third output is bf16(out + key_pe)).
    -> out [P, N, 256] (parts: also the attention output before and after the cast and the pre-norm sum)"""
    P = ktok.shape[0]
    x = _d(xin).expand(P, -1, -1)
    q = r(linear(x, Wq, bq, r))
    k, v = r(_d(ktok) * scale), r(_d(vtok))
    B, N, _ = q.shape
    sep = lambda t: t.reshape(B, t.shape[1], HEADS, CI // HEADS).transpose(1, 2)
    prob = r(torch.softmax(sep(q) @ sep(k).transpose(-1, -2), -1))
    a0 = (prob @ sep(v)).transpose(1, 2).reshape(B, N, CI)
    a = _bf(a0) if cast else a0
    y = _d(res).expand(P, -1, -1) + linear(a, Wo, bo, r)
    out = layer_norm(y, lnw, lnb, eps)
    return (out, a0, a, y) if parts else out


def kv_proj(xk, xv, Wk, bk, Wv, bv):
    """ullsam_kv_proj: the token -> image attention's k / v projections of the image side (Attention.forward transformer.py:222-223); bf16 inputs, exact products"""
    return linear(_d(xk), Wk, bk), linear(_d(xv), Wv, bv)


def up1(src, w0, b0, lnw, lnb, eps):
    """ullsam_up1_ln_gelu: ConvTranspose2d(256, 64, k2, s2) as a Linear onto (ky, kx, c) -- stride = kernel, every output pixel has one tap --, LayerNorm2d
    over each output pixel's 64 channels, GELU (mask_decoder.py:53-57).  src [rows, 256], w0 [(ky, kx, c) = 256, 256] -> [rows * 4, 64]"""
    x = linear(_d(src), w0, b0).reshape(-1, 64)
    return gelu(layer_norm(x, lnw, lnb, eps))


def up2(u1, w1, b1, hyper, NB, NM, H, W, cast=True, parts=False):
    """ullsam_up2_hyper_masks: ConvTranspose2d(64, 32, k2, s2) as a Linear onto (ky2, kx2, c), GELU (mask_decoder.py:58-59), rounded to bf16 (`cast`: the
    declared rounding), and masks = hyper @ upscaled (mask_decoder.py:143-144).  u1 [NB * H * W * 4, 64], row = ((nb H + y) W + x) 4 + 2 ky + kx.
    -> masks [NB, NM, 4H, 4W] (parts: also the GELU values [NB, 4H, 4W, 32] before the cast)"""
    g0 = gelu(linear(_d(u1), w1, b1)).reshape(NB, H, W, 2, 2, 2, 2, 32)             # [nb, y, x, ky, kx, ky2, kx2, c]
    g0 = g0.permute(0, 1, 3, 5, 2, 4, 6, 7).reshape(NB, 4 * H, 4 * W, 32)          # Y = 4 y + 2 ky + ky2, X = 4 x + 2 kx + kx2
    g = _bf(g0) if cast else g0
    masks = torch.einsum("pmc,pyxc->pmyx", _d(hyper).reshape(NB, NM, 32), g)
    return (masks, g0) if parts else masks


# ---- seeded inputs (CPU generator: the CPU and the GPU test files see the same data) ----------------------------------------------------------
def _gen(*key):
    g = torch.Generator()
    g.manual_seed(int(sum((i + 1) * 7919 ** (i + 1) * int(k) for i, k in enumerate(key)) % (2 ** 31 - 1)) + 17)
    return g


def _n(g, *shape):
    return torch.randn(shape, generator=g, dtype=torch.float32)


def _w(g, o, i):
    return (_n(g, o, i) / math.sqrt(i)).bfloat16()       # about 1 / sqrt(fan_in), bf16-rounded


def _b(g, n):
    return 0.1 * _n(g, n)


def _lw(g, n):
    return 1.0 + 0.1 * _n(g, n)


TOK_T, TOK_P = (1, 4, 5, 8, 9, 16), (1, 3)


def tok_attn_case(P, T, seed=0):
    g = _gen(1, P, T, seed)
    d = dict(queries=_n(g, P, T, C), qpe=_n(g, P, T, C))
    for n in ("q", "k", "v", "o"):
        d["W" + n], d["b" + n] = _w(g, C, C), _b(g, C)
    d.update(ln_w=_lw(g, C), ln_b=_b(g, C), eps=EPS, Wq2=_w(g, CI, C), bq2=_b(g, CI))
    return d


def tok_attn_special(name):
    """the special inputs of the GPU file -> (case, skip_pe values, checked outputs): `nulls`: all five biases and both LayerNorm parameters NULL;
    `constant_row`: zero out-projection weights, no bias, no residual (skip_pe) -- queries' is ln_b exactly in every arithmetic, only q_t2i has an error"""
    if name == "nulls":
        return dict(tok_attn_case(3, 5, seed=1), bq=None, bk=None, bv=None, bo=None, bq2=None, ln_w=None, ln_b=None), (0, 1), ("queries", "q_t2i")
    assert name == "constant_row"
    d = tok_attn_case(3, 9, seed=2)
    return dict(d, Wo=torch.zeros_like(d["Wo"]), bo=None), (1,), ("q_t2i",)


TOK_ATTN_SPECIAL = ("nulls", "constant_row")


def tok_attn_args(d, skip_pe, mode, r=ident):
    return (d["queries"], d["qpe"], d["Wq"], d["bq"], d["Wk"], d["bk"], d["Wv"], d["bv"], d["Wo"], d["bo"], d["ln_w"], d["ln_b"], d["eps"], d["Wq2"], d["bq2"],
            skip_pe, mode, r)


def tok_mlp_case(P, T, seed=0):
    g = _gen(2, P, T, seed)
    return dict(queries=_n(g, P, T, C), attn=_n(g, P, T, CI), qpe=_n(g, P, T, C), Wo=_w(g, C, CI), bo=_b(g, C), ln2_w=_lw(g, C), ln2_b=_b(g, C),
                W1=_w(g, 2048, C), b1=_b(g, 2048), W2=_w(g, C, 2048), b2=_b(g, C), ln3_w=_lw(g, C), ln3_b=_b(g, C), Wk=_w(g, CI, C), bk=_b(g, CI),
                Wv=_w(g, CI, C), bv=_b(g, CI), eps=EPS)


def tok_mlp_special(name):
    """`nulls`: every bias and LayerNorm parameter NULL; `dead`: b1 = -100 under |lin1| of a few units: every hidden unit of every row is negative"""
    if name == "nulls":
        return dict(tok_mlp_case(3, 5, seed=1), bo=None, b1=None, b2=None, bk=None, bv=None, ln2_w=None, ln2_b=None, ln3_w=None, ln3_b=None)
    assert name == "dead"
    d = tok_mlp_case(3, 9, seed=2)
    return dict(d, b1=torch.full_like(d["b1"], -100.0))


TOK_MLP_SPECIAL = ("nulls", "dead")


def tok_mlp_args(d, do_mlp, r=ident):
    return (d["queries"], d["attn"], d["qpe"], d["Wo"], d["bo"], (d["ln2_w"], d["ln2_b"], d["eps"]), d["W1"], d["b1"], d["W2"], d["b2"],
            (d["ln3_w"], d["ln3_b"], d["eps"]), d["Wk"], d["bk"], d["Wv"], d["bv"], do_mlp, r)


HEADS_CASES = [  # (P, T, m0, nm, n_iou): every P, T, (m0, nm) and n_iou of the list at least once
    (1, 5, 0, 4, 4), (16, 7, 1, 3, 4), (17, 16, 0, 1, 1), (33, 5, 3, 1, 4), (33, 7, 0, 4, 1), (16, 16, 1, 3, 1)]


def heads_case(P, T, n_iou, seed=0):
    g = _gen(3, P, T, n_iou, seed)
    hs = _n(g, P, T, C)
    chains = [[(_w(g, C, C), _b(g, C)), (_w(g, C, C), _b(g, C)), (_w(g, 32 if c < 4 else n_iou, C), _b(g, 32 if c < 4 else n_iou))] for c in range(5)]
    return hs, chains


def heads_null_case(chain):
    """P = 17, T = 7, all four masks, n_iou = 4, the three biases of `chain` NULL -> (hs, chains with None biases)"""
    hs, chains = heads_case(17, 7, 4, seed=1)
    return hs, [[(W, None if c == chain else b) for W, b in ch] for c, ch in enumerate(chains)]


HEADS_NULL_CHAINS = (2, 4)


I2T_CASES = [  # (P, N, T, shared)
    (1, 5, 1, False), (1, 5, 4, True), (3, 200, 5, False), (3, 200, 16, True), (3, 200, 15, False), (257, 275, 15, True), (257, 275, 4, False),
    (64, 1024, 16, True), (64, 1024, 5, False)]


def i2t_case(P, N, T, shared, seed=0, offset=0.0):
    """offset: a common offset of every residual row only (row mean ~ offset, spread ~ 1): norm4's variance must be two-pass"""
    g = _gen(4, P, N, T, int(shared), seed)
    B = 1 if shared else P
    keys, key_pe = _n(g, B, N, C), _n(g, N, C)
    return dict(xin=(keys + key_pe).bfloat16(), res=keys + offset, Wq=_w(g, CI, C), bq=_b(g, CI), ktok=_n(g, P, T, CI), vtok=_n(g, P, T, CI), Wo=_w(g, C, CI), bo=_b(g, C),
                lnw=_lw(g, C), lnb=_b(g, C), eps=EPS, key_pe=key_pe, scale=0.25)


I2T_SPECIAL = {  # name: (P, N, T, shared)
    "nulls": (3, 200, 15, True), "offset50": (3, 200, 5, False), "offset200": (3, 200, 5, False)}


def i2t_special(name):
    """`nulls`: bq, bo, lnw, lnb NULL; `offset50` / `offset200`: res = keys + 50 / + 200 (row mean ~ offset, spread ~ 1): a one-pass variance
    (E[x^2] - mean^2 in fp32) loses offset^2 * 2^-24 = 1.5e-4 / 2.4e-3 of a variance of ~1 per rounding of its sums"""
    P, N, T, shared = I2T_SPECIAL[name]
    if name == "nulls":
        return dict(i2t_case(P, N, T, shared, seed=2), bq=None, bo=None, lnw=None, lnb=None)
    return i2t_case(P, N, T, shared, seed=3, offset=float(name[len("offset"):]))


def i2t_prompts(d, n):
    """the first n prompts of an i2t case (same N, T, weights): the error statistics do not depend on P"""
    cut = lambda t: t if t.shape[0] == 1 else t[:n].contiguous()
    return dict(d, xin=cut(d["xin"]), res=cut(d["res"]), ktok=d["ktok"][:n].contiguous(), vtok=d["vtok"][:n].contiguous())


def norm4_one_pass_fp32(y, lnw, lnb, eps):
    """what a ONE-pass fp32 LayerNorm (variance = E[x^2] - mean^2, pairwise fp32 sums: the most accurate summation order a kernel could use) would make of
    the float64 pre-norm sum y -- the mistake the offset inputs are there to catch"""
    x = y.to(torch.float32)
    mean = x.mean(-1, keepdim=True)
    var = (x * x).mean(-1, keepdim=True) - mean * mean
    out = (x - mean) * torch.rsqrt(var.clamp(min=0) + eps)
    if lnw is not None:
        out = out * lnw.to(torch.float32)
    if lnb is not None:
        out = out + lnb.to(torch.float32)
    return out


def i2t_args(d, r=ident, cast=True, parts=False):
    return (d["xin"], d["res"], d["Wq"], d["bq"], d["ktok"], d["vtok"], d["Wo"], d["bo"], d["lnw"], d["lnb"], d["eps"], d["key_pe"], d["scale"], r, cast, parts)


def i2t_selection_case(P, N, T, seed=0):
    """Exact-selection inputs: every (row, head) attends to ONE token, so the attention output is that token's (bf16-representable) value and its cast to
    bf16 cannot flip.  The rows' inputs are solved (least squares through the random Wq, then rounded to bf16) so that head h of row n has q ~ 8 on dim
    w(n, h) < T and ~ 0 elsewhere; token t's key in every head is 64 e_t: the winner's logit leads by ~128 (asserted by the tests from the definition).
    For T < 16 dim 15 of every head carries a common -96 * 8 * scale on every real token, so a token >= T that were NOT masked (zero key, logit 0) would win.
    T = 1: one token, q free (random): the result must not depend on q at all."""
    d = i2t_case(P, N, T, False, seed=seed + 100)
    g = _gen(5, P, N, T, seed)
    d["vtok"] = d["vtok"].bfloat16().float()
    if T == 1:
        return d, None
    hd = CI // HEADS
    win = torch.randint(0, T, (P, N, HEADS), generator=g)
    qt = torch.zeros(P, N, HEADS, hd, dtype=F64)
    qt.scatter_(-1, win[..., None], 8.0)
    k = torch.zeros(P, T, HEADS, hd)
    k[:, torch.arange(T), :, torch.arange(T)] = 64.0
    if T < 16:
        qt[..., 15] = 8.0
        k[..., 15] = -96.0
    rhs = qt.reshape(P, N, CI) - d["bq"].double()
    x = rhs @ torch.linalg.pinv(d["Wq"].double()).T                  # minimum-norm rows with x Wq^T = rhs
    d["xin"] = x.float().bfloat16()
    d["ktok"] = k.reshape(P, T, CI)
    return d, win


def selection_margin(d):
    """smallest lead of the winning logit over the runner-up (natural-log units) over every (row, head), from the definition; and the winners"""
    q = linear(_d(d["xin"]), d["Wq"], d["bq"])
    P, N, _ = q.shape
    sep = lambda t: t.reshape(P, t.shape[1], HEADS, CI // HEADS).transpose(1, 2)
    s = sep(q) @ sep(_d(d["ktok"]) * d["scale"]).transpose(-1, -2)            # [P, heads, N, T]
    top = s.topk(2, -1)
    return float((top.values[..., 0] - top.values[..., 1]).min()), float(top.values[..., 0].max()), top.indices[..., 0].transpose(1, 2)


def kv_case(rows, seed=0):
    g = _gen(6, rows, seed)
    return dict(xk=_n(g, rows, C).bfloat16(), xv=_n(g, rows, C).bfloat16(), Wk=_w(g, CI, C), bk=_b(g, CI), Wv=_w(g, CI, C), bv=_b(g, CI))


def up1_case(rows, seed=0):
    g = _gen(7, rows, seed)
    return dict(src=_n(g, rows, C).bfloat16(), w0=_w(g, C, C), b0=_b(g, C), lnw=_lw(g, 64), lnb=_b(g, 64), eps=1e-6)


def up2_case(NB, H, W, NM, seed=0):
    g = _gen(8, NB, H, W, NM, seed)
    return dict(u1=_n(g, NB * H * W * 4, 64).bfloat16(), w1=_w(g, 128, 64), b1=_b(g, 128), hyper=_n(g, NB, NM, 32))


def to(d, device):
    """a case's tensors on `device` (tuples / lists / dicts walked)"""
    if torch.is_tensor(d):
        return d.to(device)
    if isinstance(d, dict):
        return {k: to(v, device) for k, v in d.items()}
    if isinstance(d, (list, tuple)):
        return type(d)(to(v, device) for v in d)
    return d


# ---- error measures ---------------------------------------------------------------------------------------------------------------------------
def err(a, ref):
    """(max |a - ref|, rms(a - ref)) in float64"""
    e = _d(a) - ref
    return float(e.abs().max()), float(torch.sqrt((e * e).mean()))


def bf16_ulp(x):
    """the spacing of bf16 at |x| (8 significant bits): 2^(floor(log2 |x|) - 7); 0 at 0"""
    a = x.abs()
    e = torch.floor(torch.log2(a.clamp(min=1e-300)))
    return torch.where(a > 0, torch.exp2(e - 7), torch.zeros_like(a))


U24 = 2.0 ** -24


def i2t_bound(d, flips=True):
    """Elementwise bound of |kernel - D| for ullsam_i2t_block's fp32 output, from the definition alone.
    Pre-norm sum y = res + bo + sum_k Wo[c, k] a[k] (128 terms):
      flips : every element of the bf16-cast attention output may sit one bf16 step off (a value on the other side of a rounding boundary):
              sum_k |Wo[c, k]| ulp_bf16(a[k]);
      fp32  : a sum of 130 fp32 terms in any order is within 130 * 2^-24 of sum |terms| (sum_k |Wo a| + |res| + |bo|).
    B = flips + fp32.  Through the LayerNorm out = w xhat + b, xhat = (y - mean) rstd: |d out| <= rstd |w| (B + mean B + |xhat| mean(|xhat| B)) (the
    derivative of xhat: d xhat_c = rstd (dy_c - mean dy - xhat_c mean(xhat dy))), plus the LayerNorm's own fp32 arithmetic (mean, variance, rsqrt, scale,
    shift: a few roundings each of the 256-term statistics) 32 * 2^-24 (|w xhat| + |b|) + the project's 2e-5-class floor 2e-6.
    Without flips (exact-selection inputs) only the fp32 terms remain."""
    out, a0, a, y = i2t(*i2t_args(d, ident, True, True))
    Wo = d["Wo"].double().abs()
    P = a.shape[0]
    res = _d(d["res"]).expand(P, -1, -1).abs()
    bo = 0.0 if d["bo"] is None else d["bo"].double().abs()
    B = 130 * U24 * (a.abs() @ Wo.T + res + bo)
    if flips:
        B = B + bf16_ulp(a) @ Wo.T
    mu = y.mean(-1, keepdim=True)
    dy = y - mu
    rstd = 1.0 / torch.sqrt((dy * dy).mean(-1, keepdim=True) + d["eps"])
    xh = dy * rstd
    w = torch.ones_like(xh) if d["lnw"] is None else d["lnw"].double().abs().expand_as(xh)
    b = 0.0 if d["lnb"] is None else d["lnb"].double().abs()
    return rstd * w * (B + B.mean(-1, keepdim=True) + xh.abs() * (xh.abs() * B).mean(-1, keepdim=True)) + 32 * U24 * (w * xh.abs() + b) + 2e-6


BF16_STEP = 2.0 ** -8


def bf16_bound(ref64, f32_bound):
    """one bf16 rounding (2^-8 relative, worst case) of an fp32 result that is itself within f32_bound of the float64 value"""
    return ref64.abs() * BF16_STEP + f32_bound


def kv_bound(x, W, b, want):
    """bf16 output of an fp32 sum of 256 exact products + bias: 257 * 2^-24 of sum |terms| (any order), then one bf16 rounding"""
    s = x.double().abs() @ W.double().abs().T + (0.0 if b is None else b.double().abs())
    return bf16_bound(want, 257 * U24 * s)


def up1_bound(d, b0, lnw, lnb, want):
    """the convolution's fp32 sums (257 * 2^-24 of sum |terms|) through the LayerNorm over 64 channels (derivative as in decoder_ref.i2t_bound), the
    LayerNorm's own fp32 arithmetic (the project's 2e-5 bound for fp32 LayerNorm chains, relative to max(1, |value|)), GELU (slope <= 1.13; the kernel's
    one-transcendental form is within 1.9e-6 of the erf form), one bf16 rounding"""
    x = linear(d["src"].double(), d["w0"], b0).reshape(-1, 64)
    B = (257 * U24 * (d["src"].double().abs() @ d["w0"].double().abs().T + (0.0 if b0 is None else b0.double().abs()))).reshape(-1, 64)
    dx = x - x.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt((dx * dx).mean(-1, keepdim=True) + d["eps"])
    xh = dx * rstd
    w = torch.ones_like(xh) if lnw is None else lnw.double().abs().expand_as(xh)
    xn = layer_norm(x, lnw, lnb, d["eps"])
    e = rstd * w * (B + B.mean(-1, keepdim=True) + xh.abs() * (xh.abs() * B).mean(-1, keepdim=True)) + 2e-5 * xn.abs().clamp(min=1.0)
    return bf16_bound(want, 1.13 * e + 1.9e-6)


def up2_bound(d, b1, NB, NM, H, W):
    """sum_c |h_c| (2^-8 |gelu_c| + fp32 term of gelu_c) + the fp32 dot product (33 * 2^-24 of sum |h gelu|); the fp32 term of a channel: its 64-term sum
    (65 * 2^-24 of sum |terms|) through GELU (slope <= 1.13) + 1.9e-6 (the one-transcendental GELU), carried through the rounding ((1 + 2^-8) x).
    The reference is the definition WITHOUT the declared cast: the bound holds the cast's rounding."""
    _, g0 = up2(d["u1"], d["w1"], b1, d["hyper"], NB, NM, H, W, cast=False, parts=True)
    s = d["u1"].double().abs() @ d["w1"].double().abs().T + (0.0 if b1 is None else b1.double().abs())
    f = (1.13 * 65 * U24 * s + 1.9e-6).reshape(NB, H, W, 2, 2, 2, 2, 32).permute(0, 1, 3, 5, 2, 4, 6, 7).reshape(NB, 4 * H, 4 * W, 32)
    per = BF16_STEP * g0.abs() + (1 + BF16_STEP) * f
    h = d["hyper"].double().abs().reshape(NB, NM, 32)
    return torch.einsum("pmc,pyxc->pmyx", h, per) + 33 * U24 * torch.einsum("pmc,pyxc->pmyx", h, g0.abs())
