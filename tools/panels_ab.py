"""The ring GEMM reading its weight as K-panels (packing.pack_ring_panels, ullsam_set_gemm_tuning(4, 1)) against the same launch reading the
row-major weight (4, 0), ONE process: bit-equality of the outputs, then interleaved timing rounds on cold operands (as tools/persist_ab.py).
Three modes per shape: `rm` and `rm2` are both the row-major weight -- their difference is the noise floor of this run (A/A) -- and `pn` the panels.
usage: python tools/panels_ab.py [rounds]          GEMM_SHAPES=name,name restricts the shapes; PANELS_MODES=rm (or pn) runs ONE layout only and prints its median
(a counter pass under rocprofv3 --pmc: one layout per process, so that every dispatch of a kernel name in the counter file is of that layout)
PANELS_KIND=act: the same A/B for the ACTIVATIONS (packing.pack_activation_panels, ullsam_set_gemm_tuning(5, v)): `rm` / `rm2` read A and write C row-major, `pn` reads A as
panels and writes C as panels wherever the library's query says the launch can (weights as panels throughout, the default); then the two norm kernels writing row-major / panels"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ullsam_amd import ops, _lib
from ullsam_amd.packing import pack_activation_panels, pack_ring_panels, unpack_activation_panels

lib = _lib.load()
dev = "cuda"
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
MODES = [("rm", 0), ("rm2", 0), ("pn", 1)]
ACT = os.environ.get("PANELS_KIND") == "act"
KEY = 5 if ACT else 4
if os.environ.get("PANELS_MODES"):
    MODES = [m for m in MODES if m[0] in os.environ["PANELS_MODES"].split(",")]
SHAPES = [  # name, M, N, K, act (4: wqkv + RoPE epilogue), bias, fp32 residual      -- the eight GEMM classes of the bench step, then the plain forms
    ("llm.w13", 4324, 28672, 4096, 3, False, False), ("llm.wqkv+rope", 4324, 6144, 4096, 4, False, False), ("llm.wo+r", 4324, 4096, 4096, 0, False, True),
    ("llm.w2+r", 4324, 4096, 14336, 0, False, True), ("vit.qkv", 16384, 3840, 1280, 0, True, False), ("vit.lin1", 16384, 5120, 1280, 1, True, False),
    ("vit.proj+r", 16384, 1280, 1280, 0, True, True), ("vit.lin2+r", 16384, 1280, 5120, 0, True, True),
    ("llm.w13.plain", 4324, 28672, 4096, 0, False, False), ("llm.wqkv.plain", 4324, 6144, 4096, 0, False, False),
]


def med(v):
    return sorted(v)[len(v) // 2]


def main():
    only = os.environ.get("GEMM_SHAPES")
    print(f"{'shape':16s} {'M':>6s} {'N':>6s} {'K':>6s} | row-major us (min..max) | A/A us   % | panels us (min..max)   % | bit-equal", flush=True)
    for name, M, N, K, act, hb, res in SHAPES:
        if only and name not in only.split(","):
            continue
        n_out = N // 2 if act == 3 else N
        ncopy = max(2, int(6e8 // (2 * (M * K + N * K * 2 + M * n_out))) + 1)
        As = [torch.randn(M, K, device=dev).bfloat16() for _ in range(ncopy)]
        Ws = [(torch.randn(N, K, device=dev) * K ** -0.5).bfloat16() for _ in range(ncopy)]
        Ps = [pack_ring_panels(w) for w in Ws]
        bias = torch.randn(N, device=dev) if hb else None
        APs, ra, wc = None, False, False
        if ACT:
            with torch.no_grad():
                ra, wc = ops.activation_panels_plan(M, N, K, torch.bfloat16, act=act, out_f32=res, bias=hb, residual=res, rope=act == 4)
            APs = [pack_activation_panels(a) for a in As] if ra else None
        on = [False]   # the mode being run reads / writes activation panels
        if act == 4:
            B, S, KVH, G = 4, M // 4, 8, 4
            assert N == KVH * (G + 2) * 128
            pos = torch.arange(S, device=dev, dtype=torch.int32).repeat(B)
            ang = torch.arange(S, device=dev, dtype=torch.float32)[:, None] * torch.exp(-torch.arange(64, device=dev, dtype=torch.float32) / 64 * 9.2)[None]
            cos, sin = torch.cat([ang.cos(), ang.cos()], 1).contiguous(), torch.cat([ang.sin(), ang.sin()], 1).contiguous()
            kc = [torch.zeros(B, KVH, S, 128, device=dev, dtype=torch.bfloat16) for _ in range(2)]

            def run(i, out):
                ap = on[0] and ra
                return ops.gemm_qkv_rope(APs[i] if ap else As[i], Ws[i], None, kc[0], kc[1], pos, cos, sin, B, S, KVH, G, 0, w_panels=Ps[i], a_panels=ap)
        else:
            def run(i, out):
                ap, cp = on[0] and ra, on[0] and wc
                return ops.gemm(APs[i] if ap else As[i], Ws[i], bias, act=act, out=None if cp else out, out_f32=res, residual=out if res else None, w_panels=Ps[i],
                                a_panels=ap, out_panels=cp, m=M)
        outs = {}
        for mname, v in MODES:
            lib.ullsam_set_gemm_tuning(KEY, v)
            on[0] = ACT and v == 1
            o = torch.arange(M * N, device=dev, dtype=torch.float32).reshape(M, N) * 1e-6 if res else None
            o = run(0, o)
            if on[0] and wc:
                o = unpack_activation_panels(o, M)
            outs[mname] = [o.clone()] + ([kc[0].clone(), kc[1].clone()] if act == 4 else [])
        torch.cuda.synchronize()
        eq = all(torch.equal(x, y) for x, y in zip(outs["rm"], outs["pn"])) if len(MODES) == 3 else None
        Cs = [torch.zeros(M, n_out, device=dev, dtype=torch.float32 if res else torch.bfloat16) for _ in range(ncopy)]
        times = {m: [] for m, _ in MODES}
        for r in range(rounds):
            order = MODES[r % len(MODES):] + MODES[:r % len(MODES)]
            for mname, v in order:
                lib.ullsam_set_gemm_tuning(KEY, v)
                on[0] = ACT and v == 1
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(ncopy):
                    run(i, Cs[i])
                e1.record()
                torch.cuda.synchronize()
                times[mname].append(e0.elapsed_time(e1) / ncopy * 1e3)
        if len(MODES) != 3:
            print(f"{name:16s} {M:6d} {N:6d} {K:6d} | " + " | ".join(f"{m}: {med(times[m]):8.1f} us" for m, _ in MODES), flush=True)
            del As, Ws, Ps, Cs, APs
            continue
        t0, t1, t2 = med(times["rm"]), med(times["rm2"]), med(times["pn"])
        print(f"{name:16s} {M:6d} {N:6d} {K:6d} | {t0:8.1f} ({min(times['rm']):.1f}..{max(times['rm']):.1f}) | {t1:8.1f} {100 * (t1 / t0 - 1):+5.2f} | "
              f"{t2:8.1f} ({min(times['pn']):.1f}..{max(times['pn']):.1f}) {100 * (t2 / t0 - 1):+5.2f} | {eq}", flush=True)
        del As, Ws, Ps, Cs, APs
    lib.ullsam_set_gemm_tuning(KEY, 1)
    if ACT:
        norms()


def norms():
    """The producers: RMSNorm [4324, 4096] (norm_block_kernel) and LayerNorm [16384, 1280] (norm_kernel), fp32 -> bf16, row-major against panels, cold inputs."""
    for name, rows, D, rms in (("llm.rmsnorm", 4324, 4096, True), ("vit.layernorm", 16384, 1280, False)):
        ncopy = max(2, int(6e8 // (6 * rows * D)) + 1)
        Xs = [torch.randn(rows, D, device=dev) for _ in range(ncopy)]
        w, b = torch.randn(D, device=dev), None if rms else torch.randn(D, device=dev)
        eq = torch.equal(ops.norm(Xs[0], w, b, 1e-6, torch.bfloat16, rms=rms), unpack_activation_panels(ops.norm(Xs[0], w, b, 1e-6, torch.bfloat16, rms=rms, out_panels=True), rows))
        times = {m: [] for m, _ in MODES}
        for r in range(rounds):
            for mname, v in MODES[r % len(MODES):] + MODES[:r % len(MODES)]:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(ncopy):
                    ops.norm(Xs[i], w, b, 1e-6, torch.bfloat16, rms=rms, out_panels=v == 1)
                e1.record()
                torch.cuda.synchronize()
                times[mname].append(e0.elapsed_time(e1) / ncopy * 1e3)
        print(f"{name:16s} {rows:6d} {D:6d} {'':6s} | " + " | ".join(f"{m}: {med(times[m]):8.1f} us ({min(times[m]):.1f}..{max(times[m]):.1f})" for m, _ in MODES) + f" | {eq}", flush=True)


if __name__ == "__main__":
    main()
