"""Times the half-pair GEMM on the big shapes of a training step with the library RNNT_HIP_LIB points at (default: the in-tree build).
   python tools/gemm_hp_time.py [label] [--step-shapes]      (one process per library variant: tools/gemm_hp_bound_probe.sh,
                                                              tools/gemm_hp_epilogue_ab.sh)
   default: the three big c2 shapes.  --step-shapes: also the step's other shapes (the K = 80 layer-0 projection, which is almost pure
   epilogue; a split-K weight gradient; the out_proj-sized product; c5's projection) and one machine-readable line `#us label name=us ...`.
   proj and dX have the same FLOPs and the same number of K-tiles but 8 against 2 rounds of 256 x 256 tiles on 256 CUs: (proj - dX) / 6 is
   the cost of a round that does not depend on K."""
import os, sys, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from rnntransducer_amd.ops import gemm_hp, hp_split
args = [a for a in sys.argv[1:] if not a.startswith("--")]
label = args[0] if args else "default"
shapes = [("proj", (32000, 4096, 1024)), ("dX", (32000, 1024, 4096)), ("dW", (4096, 1024, 32000))]
if "--step-shapes" in sys.argv:
    shapes += [("proj0", (32000, 4096, 80)), ("dWout", (2048, 512, 32000)), ("out", (32000, 512, 1024)), ("c5proj", (24000, 5120, 1280))]
dev = "cuda"
g = torch.Generator(device=dev).manual_seed(0)
out_line, us = [], []
for name, (M, N, K) in shapes:
    a = hp_split(torch.randn(M, K, device=dev, generator=g))
    b = hp_split(torch.randn(N, K, device=dev, generator=g) * 0.05)
    out = torch.empty(M, N, device=dev)
    ts = []
    for r in range(6):
        gemm_hp(a, b, out); torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(5):
            gemm_hp(a, b, out)
        e1.record(); torch.cuda.synchronize()
        if r: ts.append(e0.elapsed_time(e1) / 5)
    t = statistics.median(ts)
    out_line.append(f"{name} {1e3 * t:.0f} us ({2.0 * M * N * K / t / 1e9:.0f} TF-equivalent)")
    us.append(f"{name}={1e3 * t:.1f}")
    del a, b, out
print(f"{label:>28} | " + " | ".join(out_line), flush=True)
if "--step-shapes" in sys.argv:
    print(f"#us {label} " + " ".join(us), flush=True)
