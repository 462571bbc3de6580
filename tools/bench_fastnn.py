#!/usr/bin/env python3
"""Fast reciprocal NN (K8) in isolation: P pairs of 512 x 512 fp16 / fp32 descriptor maps, 64 x 64 seeds, 3 rounds.
Times one matcher call (matching.fast_reciprocal_nn_maps) with the block-bound search (prune=True) and with brute force
(prune=False), prints the device time of every round (m3_frnn_round_pruned x 3; m3_frnn_round, then m3_frnn_round_active
x 2) and the MFMA rate of a brute-force search, and ends with the same figures as one JSON line.
    python tools/bench_fastnn.py [--pairs P] [--reps R]"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "mast3r-slam_amd")]
import torch
from mast3r_slam import _ffi, matching, synthetic


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


P, REPS = arg("--pairs", 8), arg("--reps", 5)
ROUNDS = ("m3_frnn_round", "m3_frnn_round_active", "m3_frnn_round_pruned")
dev = torch.device("cuda:0")
H = W = 512
sc = synthetic.geometric_pair(H, W, seed=1000, batch=P)
D1 = torch.from_numpy(sc["D21"]).to(dev)
D2 = torch.from_numpy(sc["D11"]).to(dev)
med = lambda v: sorted(v)[len(v) // 2]
result = {"pairs": P, "reps": REPS}
for half in (True, False):
    a, b = (D1.half(), D2.half()) if half else (D1, D2)
    for prune in (True, False):
        for _ in range(2):
            matching.fast_reciprocal_nn_maps(a, b, subsample=8, max_iter=3, tracker_maps=False, prune=prune)
        torch.cuda.synchronize()
        _ffi.PROFILE, _ffi.PROFILE_NAMES = {}, ROUNDS
        calls = []
        for _ in range(REPS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = matching.fast_reciprocal_nn_maps(a, b, subsample=8, max_iter=3, tracker_maps=False, prune=prune)
            e1.record()
            calls.append((e0, e1))
        torch.cuda.synchronize()
        prof, _ffi.PROFILE = _ffi.PROFILE, None
        us = lambda name: [x.elapsed_time(y) * 1e3 for x, y in prof.get(name, [])]
        # the rounds of a call in order: three pruned ones, or the full round and two active ones
        seq = us("m3_frnn_round_pruned") if prune else \
            [u for r in range(REPS) for u in [us("m3_frnn_round")[r]] + us("m3_frnn_round_active")[2 * r:2 * r + 2]]
        rounds = [med(seq[r::3]) for r in range(3)]
        call_us = med([x.elapsed_time(y) * 1e3 for x, y in calls])
        tag = f"{'fp16' if half else 'fp32'} {'pruned' if prune else 'brute'}"
        result[tag.replace(" ", "_")] = {"call_us": round(call_us, 1), "round_us": [round(u, 1) for u in rounds]}
        line = f"{tag:12s} {P} pairs: matcher call {call_us:.0f} us, rounds " + " / ".join(f"{u:.0f}" for u in rounds) + " us"
        if not prune:
            fl = 2.0 * P * out["seeds"] * H * W * 24                  # one search; the full round runs two
            line += f" -> {2 * fl / rounds[0] / 1e6:.0f} TFLOP/s per search (D = 24)"
        print(line + f", {int(out['count'].sum())} reciprocal pairs")
print(json.dumps(result))
