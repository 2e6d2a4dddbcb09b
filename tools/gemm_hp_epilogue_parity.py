"""Bitwise comparison of two builds of the library (the in-tree one against OTHER, e.g. the parent commit built in a
git worktree): one fresh process per library, results as .npy files, compared byte for byte.
   python tools/gemm_hp_epilogue_parity.py OTHER.so OUTDIR [--bench]
   products: every product of tests/test_gpu_gemm_hp_epilogue.py (RNNT_HP_EPILOGUE_DUMP)
   --bench:  also `bench.py --config c2 --steps 3 --warmup 1 --dump-outputs` (a training step is bitwise reproducible)
Exit status 1 when a file differs or is missing on one side, or a child fails (nothing more is started then)."""
import os, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(cmd, env_extra, limit):
    env = dict(os.environ, **env_extra)
    if not env.get("RNNT_HIP_LIB"):
        env.pop("RNNT_HIP_LIB", None)
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        print(r.stdout[-3000:])
        sys.exit(f"FAILED ({r.returncode}): {' '.join(cmd)}")
    return r.stdout


def compare(a, b, what):
    names = sorted(set(os.listdir(a)) | set(os.listdir(b)))
    bad = 0
    for n in names:
        pa, pb = os.path.join(a, n), os.path.join(b, n)
        if not (os.path.exists(pa) and os.path.exists(pb)):
            print(f"{what}: {n} MISSING on one side"); bad += 1
        elif open(pa, "rb").read() != open(pb, "rb").read():
            print(f"{what}: {n} DIFFERS"); bad += 1
    print(f"{what}: {len(names)} files, {len(names) - bad} bytewise equal, {bad} differ")
    return bad


def main():
    other, out = os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])
    bad = 0
    libs = (("other", other), ("main", ""))
    for tag, lib in libs:
        run([sys.executable, "-m", "pytest", "tests/test_gpu_gemm_hp_epilogue.py", "-q", "-x", "-m", "gpu"],
            {"RNNT_HIP_LIB": lib, "RNNT_HP_EPILOGUE_DUMP": os.path.join(out, "products_" + tag)}, 300)
    bad += compare(os.path.join(out, "products_other"), os.path.join(out, "products_main"), "test products")
    if "--bench" in sys.argv:
        for tag, lib in libs:
            run([sys.executable, "bench.py", "--config", "c2", "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--dump-outputs",
                 os.path.join(out, "bench_" + tag)], {"RNNT_HIP_LIB": lib}, 300)
        bad += compare(os.path.join(out, "bench_other"), os.path.join(out, "bench_main"), "bench c2 outputs")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
