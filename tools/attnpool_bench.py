"""Times CLIP's attention pooling (tris_amd.CLIP.clip.model.AttentionPool2d, csrc/attnpool.hip) on the GPU:

    python tools/attnpool_bench.py [--out profiles/attnpool_bench.jsonl] [--reps 7] [--inner 20] [--batch 48]

Shape: the RN50 training shape, B = 48 images of 320 px: c4 [48, 10, 10, 2048] channels-last, L = 101 tokens, 32 heads, out 1024.
Three cases on the same seeded module and input:
* full      -- AttentionPool2d.forward: tokens kernel, ONE [3C, C] product over B L rows, ops.mha, c_proj over B L rows;
* folded    -- forward(global_only=True): tokens kernel, q_proj on B rows, two per-head products of B rows, the pool kernel, c_proj on B rows;
* torch     -- the reference's forward restated in torch on the same device (F.interpolate, F.multi_head_attention_forward with separate
               projection weights, CLIP/clip/model.py:70-104): what the op costs without this package's kernels.
The two kernels are timed alone as well, with the bytes they must move over that time.  Outputs are compared before anything is timed.

A timed window is `inner` back-to-back calls between two HIP events on the current stream, after a warm-up of the same shapes; the
median of `reps` windows divided by `inner` is reported in microseconds per call.  One JSON line per row.
"""
import argparse
import json
import os
import sys

os.environ.setdefault("TRIS_RANDOM_INIT", "1")
import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

C, HEADS, OUT, S, HW = 2048, 32, 1024, 7, 10


def window(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner


def timed(fn, reps, inner, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    return float(np.median([window(fn, inner) for _ in range(reps)]))


def torch_forward(m, x):
    """the reference's AttentionPool2d.forward on an NCHW tensor, in torch ops"""
    B, Cc, H, W = x.shape
    t = x.reshape(B, Cc, H * W).permute(2, 0, 1)
    t = torch.cat([t.mean(dim=0, keepdim=True), t], dim=0)
    pe = m.positional_embedding
    sp = F.interpolate(pe[1:].reshape(1, S, S, Cc).permute(0, 3, 1, 2), size=(H, W), mode="bilinear")
    t = t + torch.cat([pe[0:1], sp.reshape(Cc, H * W).permute(1, 0)], dim=0)[:, None, :]
    t, _ = F.multi_head_attention_forward(
        query=t, key=t, value=t, embed_dim_to_check=Cc, num_heads=HEADS, q_proj_weight=m.q_proj.weight, k_proj_weight=m.k_proj.weight,
        v_proj_weight=m.v_proj.weight, in_proj_weight=None, in_proj_bias=torch.cat([m.q_proj.bias, m.k_proj.bias, m.v_proj.bias]),
        bias_k=None, bias_v=None, add_zero_attn=False, dropout_p=0, out_proj_weight=m.c_proj.weight, out_proj_bias=m.c_proj.bias,
        use_separate_proj_weight=True, training=False, need_weights=False)
    t = t.permute(1, 2, 0)
    return t[:, :, 0], t[:, :, 1:].reshape(B, -1, H, W)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", default=7, type=int)
    ap.add_argument("--inner", default=20, type=int)
    ap.add_argument("--batch", default=48, type=int)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "attnpool_bench needs the MI355X"
    from tris_amd import ops
    from tris_amd.CLIP.clip.model import AttentionPool2d
    B, L = args.batch, HW * HW + 1
    torch.manual_seed(5)
    m = AttentionPool2d(S, C, HEADS, OUT)
    with torch.no_grad():
        for p in (m.q_proj, m.k_proj, m.v_proj, m.c_proj):
            p.weight.normal_(std=C ** -0.5)
            p.bias.normal_(std=0.1)
    m = m.cuda().eval()
    x = torch.randn(B, HW, HW, C).relu_().cuda()                    # c4 is the output of a ReLU
    x_nchw = x.permute(0, 3, 1, 2).contiguous()
    rows = []
    with torch.no_grad():
        glob, fmap = m(x)
        g_only = m(x, global_only=True)
        ref_g, ref_f = torch_forward(m, x_nchw)
        scale = float(ref_g.abs().max())
        agree = {"full_vs_torch": float((glob - ref_g).abs().max()) / scale, "folded_vs_torch": float((g_only - ref_g).abs().max()) / scale,
                 "feature_map_vs_torch": float((fmap - ref_f).abs().max()) / float(ref_f.abs().max())}
        base = {"B": B, "c4": f"{HW}x{HW}x{C}", "L": L, "heads": HEADS, "out": OUT, "gemm_mode": ops.get_gemm_mode()}
        cases = [("full", lambda: m(x)), ("folded", lambda: m(x, global_only=True)), ("torch", lambda: torch_forward(m, x_nchw))]
        for name, fn in cases:
            r = {"case": name, **base, "us_per_call": round(timed(fn, args.reps, args.inner), 2)}
            if name == "torch":
                r["max_err_over_max"] = {k: float(f"{v:.3g}") for k, v in agree.items()}
            rows.append(r)
            print(json.dumps(r), flush=True)
        # the two kernels alone
        T = ops.attnpool_tokens(x, m.positional_embedding, S)
        moved = 4 * (2 * B * HW * HW * C + B * C + (S * S + 1) * C)            # c4 in, T out, the positional table once
        r = {"case": "kernel_tokens", **base, "us_per_call": round(timed(lambda: ops.attnpool_tokens(x, m.positional_embedding, S), args.reps, args.inner), 2),
             "bytes_moved": moved}
        r["TB_per_s"] = round(moved / (r["us_per_call"] * 1e-6) / 1e12, 3)
        rows.append(r)
        print(json.dumps(r), flush=True)
        U = torch.randn(HEADS, B, C, device="cuda").mul_(0.05).transpose(0, 1)
        moved = 4 * (B * L * C + 2 * B * HEADS * C + B * HEADS * L)              # T once from HBM (its re-reads hit L2), U in, pooled and P out
        r = {"case": "kernel_pool", **base, "us_per_call": round(timed(lambda: ops.attnpool_pool(T, U, 0.125), args.reps, args.inner), 2),
             "bytes_moved": moved}
        r["TB_per_s"] = round(moved / (r["us_per_call"] * 1e-6) / 1e12, 3)
        rows.append(r)
        print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps({"device": torch.cuda.get_device_name(0), "reps": args.reps, "inner": args.inner, **r}) + "\n")


if __name__ == "__main__":
    main()
