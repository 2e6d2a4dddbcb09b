"""What the compiler made of the epilogue of hp_tile256: compiles gemm_hp.hip sources to gfx950 assembly (no GPU needed) and counts, per
kernel, behind the last MFMA: lines, vector stores and loads, vmcnt waits, division expansions (v_rcp_iflag), and the straight-line
runs of stores (no label, branch or load inside) with the waits they contain — the store-mode and slab-mode path is such a run.
   python tools/gemm_hp_epilogue_listing.py LABEL=path/to/gemm_hp.hip [LABEL=path ...]  > profiles/gemm_hp_epilogue_listing.txt"""
import os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rnntransducer_amd.csrc.build import HIPCC
KERNELS = ("gemm_hp_kernelILb0E", "gemm_hpq_kernelILb0E")


def listing(src):
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "gemm_hp.s")
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "rnntransducer_amd", "csrc"), src, "-o", out], check=True, stderr=subprocess.DEVNULL)
        return open(out).read().split("\n")


def report(label, src):
    s = listing(src)
    for k in KERNELS:
        i0 = next(i for i, l in enumerate(s) if k in l and re.match(r"_Z\S+:", l))
        i1 = next(i for i in range(i0, len(s)) if s[i].startswith(".Lfunc_end"))
        name = s[i0].split(":")[0]
        meta = next(i for i, l in enumerate(s) if ".name:" in l and name in l)
        get = lambda key: next(l.split(":")[1].strip() for l in s[meta:meta + 24] if key in l)
        body = s[i0:i1]
        ep = body[max(i for i, l in enumerate(body) if "v_mfma" in l) + 1:]
        is_store = lambda l: re.search(r"\b(buffer|global|flat)_store", l) is not None
        is_load = lambda l: re.search(r"\b(buffer|global|flat)_load", l) is not None
        runs, cur = [], None
        for l in ep:
            t = l.strip()
            if t.startswith(".LBB") or re.match(r"s_c?branch", t) or is_load(t):
                if cur and cur[0] >= 16: runs.append(cur)
                cur = None
            elif is_store(t):
                cur = cur or [0, 0, 0, 0]
                cur[0] += 1
                cur[1] += cur[2]; cur[2] = 0          # waits seen since the previous store lie between two stores
            elif cur and "vmcnt" in t:
                cur[2] += 1
            elif cur and "v_rcp_iflag" in t:
                cur[3] += 1
        if cur and cur[0] >= 16: runs.append(cur)
        print(f"{label:>8} {k.replace('ILb0E', '<false>'):24} VGPRs {get('.vgpr_count')}, scratch {get('.private_segment_fixed_size')} B, spilled VGPRs {get('.vgpr_spill_count')}")
        print(f"{'':8} behind the last MFMA: {len(ep)} lines, {sum(map(is_store, ep))} stores, {sum(map(is_load, ep))} loads, "
              f"{sum('vmcnt' in l for l in ep)} vmcnt waits, {sum(bool(re.match(r's_c?branch', l.strip())) for l in ep)} branches, "
              f"{sum('v_rcp_iflag' in l for l in ep)} division expansions")
        print(f"{'':8} straight-line runs of >= 16 stores (no label, branch or load inside): "
              + (", ".join(f"{r[0]} stores with {r[1]} vmcnt waits and {r[3]} division expansions between them" for r in runs) or "none: every store sits in a block of its own"))


if __name__ == "__main__":
    for a in sys.argv[1:]:
        label, src = a.split("=", 1)
        report(label, os.path.abspath(src))
