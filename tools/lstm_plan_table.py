"""What a build of the library decides for the recurrent layers, shape by shape: one line per shape with the answers of the shape
queries (rnnt_hip_lstm_workspace_bytes, _max_batch, _takes_row_idx, _takes_f16, _free_xcds).  They need no device (256 CUs assumed),
so two builds are compared with

    python tools/lstm_plan_table.py > new.txt;  RNNT_HIP_LIB=/path/to/other/librnnt_hip.so python tools/lstm_plan_table.py > old.txt

run plainly and under each env switch that moves a shape between kernel forms (RNNT_LSTM_V1, RNNT_LSTM_V2, RNNT_LSTM_NO_V5,
RNNT_LSTM_V5_WIDE, RNNT_LSTM_EXACT_MATH, RNNT_GEMM_NO_HP, RNNT_GEMM_FORCE_HP, RNNT_LSTM_NO_XCD_STRIDE: each `=1`).  A refactor of
the layer's host code leaves every line as it is.
"""
import ctypes
import os
import sys

HS = list(range(4, 161, 4)) + [192, 256, 320, 384, 512, 520, 640, 768, 896, 1024, 1028, 2048]
BS = [1, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65]
# the last three straddle the 2 GiB v5 stash and the 4 GB plane limits
TI = [(1, 80), (41, 31), (41, 32), (100, 127), (100, 128), (1000, 80), (1000, 1024), (2047, 1024), (2048, 1024), (2048, 2048)]


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    path = os.environ.get("RNNT_HIP_LIB") or os.path.join(here, "..", "rnntransducer_amd", "csrc", "librnnt_hip.so")
    lib = ctypes.CDLL(path)
    i32 = ctypes.c_int32
    lib.rnnt_hip_lstm_workspace_bytes.restype = ctypes.c_size_t
    lib.rnnt_hip_lstm_workspace_bytes.argtypes = [i32] * 5
    for name, n in (("max_batch", 3), ("takes_row_idx", 6), ("takes_f16", 6), ("free_xcds", 5)):
        fn = getattr(lib, "rnnt_hip_lstm_" + name)
        fn.restype, fn.argtypes = i32, [i32] * n
    out = []
    for H in HS:
        for D in (1, 2):
            for cell in range(4):
                out.append(f"H={H} D={D} cell={cell} max_batch={lib.rnnt_hip_lstm_max_batch(H, D, cell)}")
                for B in BS:
                    for T, I in TI:
                        out.append(f"H={H} D={D} cell={cell} B={B} T={T} I={I}"
                                   f" ws={lib.rnnt_hip_lstm_workspace_bytes(T, B, I, H, D)}"
                                   f" row_idx={lib.rnnt_hip_lstm_takes_row_idx(T, B, I, H, D, cell)}"
                                   f" f16={lib.rnnt_hip_lstm_takes_f16(T, B, I, H, D, cell)}"
                                   f" free_xcds={lib.rnnt_hip_lstm_free_xcds(T, B, H, D, cell)}")
    sys.stdout.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
