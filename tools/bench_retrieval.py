#!/usr/bin/env python3
"""Retrieval kernels in isolation (csrc/retrieval.hip), hipEvent timing on a warmed stream:
  signature: B in {1, 8} frames of T = 1024 tokens x C = 1024 fp16 (2 MiB per frame);
  top-k:     N in {256, 4096, 65536} stored fp32 signatures, Q in {1, 8} queries, k = 3.
Prints the median device time of one call (two launches each), the bytes it must move and the fraction of the HBM
rate (--hbm, TB/s; default 8.0, the MI355X datasheet figure) that reaches."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mast3r-slam_amd")]
import torch
from mast3r_slam import _ffi

HBM = float(sys.argv[sys.argv.index("--hbm") + 1]) if "--hbm" in sys.argv else 8.0
REPS = 50
dev = torch.device("cuda:0")
L = _ffi.lib()
st = _ffi.stream_ptr


def timed(fn):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        ts.append((e0, e1))
    torch.cuda.synchronize()
    us = sorted(a.elapsed_time(b) * 1e3 for a, b in ts)
    return us[len(us) // 2], us[0]


def row(name, us, umin, nbytes):
    gbs = nbytes / us / 1e3
    print(f"| {name} | {us:.1f} | {umin:.1f} | {nbytes / 2**20:.2f} | {gbs:.0f} | {gbs / (HBM * 1e3):.2f} |", flush=True)


print(f"device: {torch.cuda.get_device_name(0)}; HBM reference {HBM} TB/s; median of {REPS} calls")
print("| call | median us | min us | MiB moved | GB/s | of HBM |")
print("|---|---|---|---|---|---|")
T = C = 1024
for B in (1, 8):
    feat = torch.randn(B, T, C, device=dev).half()
    sig = torch.empty(B, C, device=dev)
    ws = torch.empty(L.m3_retrieval_signature_ws_bytes(B, T, C), dtype=torch.uint8, device=dev)
    f = lambda: _ffi.call("m3_retrieval_signature", feat.data_ptr(), sig.data_ptr(), C, ws.data_ptr(), ws.numel(),
                          B, T, C, 1, st())
    us, umin = timed(f)
    row(f"signature B={B} T={T} C={C} fp16", us, umin, B * T * C * 2 + B * C * 4)
k = 3
for N in (256, 4096, 65536):
    db = torch.nn.functional.normalize(torch.randn(N, C, device=dev), dim=1)
    for Q in (1, 8):
        q = db[:Q].clone()
        ws = torch.empty(L.m3_retrieval_ws_bytes(N, Q, k, 0), dtype=torch.uint8, device=dev)
        out = torch.empty(Q * (1 + 2 * k), dtype=torch.int32, device=dev)
        f = lambda: _ffi.call("m3_retrieval_topk", q.data_ptr(), C, db.data_ptr(), C, N, Q, C, k, 1, 0.005, 0,
                              out.data_ptr(), out[Q:].data_ptr(), out[Q + Q * k:].data_ptr(), ws.data_ptr(),
                              ws.numel(), st())
        us, umin = timed(f)
        row(f"top-k N={N} Q={Q} k={k}", us, umin, N * C * 4 + Q * C * 4)
