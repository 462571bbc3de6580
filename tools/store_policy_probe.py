#!/usr/bin/env python3
"""Driver of the output-store policy probe (tools/experiments/store_policy_probe.hip): what a kernel's closing burst of output
stores costs at the boundary to the next, dependent kernel, for plain and for write-through (sc1) stores.  Table in
profiles/store_policy.md.

    python tools/store_policy_probe.py --build-only     # compile for gfx950 -> tools/experiments/_build/
    python tools/store_policy_probe.py [repeats] [spin ticks of the 100 MHz wall clock]
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "experiments", "store_policy_probe.hip")
EXE = os.path.join(HERE, "experiments", "_build", "store_policy_probe")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17"]


def build(force: bool = False) -> str:
    """hipcc store_policy_probe.hip -> _build/store_policy_probe (skipped when the program is newer than the source)."""
    if not force and os.path.exists(EXE) and os.path.getmtime(EXE) >= os.path.getmtime(SRC):
        return EXE
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    tmp = f"{EXE}.{os.getpid()}.tmp"
    r = subprocess.run([hipcc, *FLAGS, SRC, "-o", tmp], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed on {SRC}:\n{r.stderr}")
    os.replace(tmp, EXE)
    return EXE


if __name__ == "__main__":
    args = sys.argv[1:]
    if args and args[0] == "--build-only":
        print(build(force=True))
        sys.exit(0)
    sys.exit(subprocess.run([build(), *args]).returncode)
