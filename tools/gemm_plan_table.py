"""The shape grid behind tests/golden/gemm_plan_makespan.txt and the plan the built library gives each shape.

    python tools/gemm_plan_table.py shapes          # M N K rpb kchunk groups flags, one product per line
    python tools/gemm_plan_table.py plan [0|1]      # the same lines + what afx_gemm_plan answers under that objective

The grid holds every dense product of both models (trunk, conv feature encoder with its fused LayerNorm epilogue, the chunked-K
positional conv, the Conformer head's unfused products, the AASIST projection) at B = 1, 7, 16, 64 and 1-s / 4-s clips, in fp16
and split precision, plus a plain grid around the thresholds of the dispatch (384 tiles of 128x128, whole rounds of 256 CUs,
tile heights 160..256).  The golden table was written from the commit BEFORE the planner existed: its dispatch functions
compiled host-only into a small program that read this grid; `plan 0` on any later commit must reproduce it line for line
(tests/test_cpu_gemm_plan.py).  No GPU is needed: the plan is host arithmetic."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "real-time-deepfake-speech-detection_amd")]

LN, S3, ACT, NO_DEEP = 1, 2, 4, 8


def conv_frames(L):
    t = [(L - 10) // 5 + 1]
    for k in (3, 3, 3, 3, 2, 2):
        t.append((t[-1] - k) // 2 + 1)
    return t  # frames after conv layers 0..6


def shapes():
    out = []
    seen = set()

    def add(M, N, K, rpb=0, kchunk=0, groups=1, flags=0):
        key = (M, N, K, rpb, kchunk, groups, flags)
        if M > 0 and key not in seen:
            seen.add(key)
            out.append(key)

    for L in (16000, 64000):
        t = conv_frames(L)
        T = t[-1]
        for B in (1, 7, 16, 64):
            for s3 in (0, S3):
                for i in range(1, 7):  # conv layers 1-6: Conv1d(512 -> 512, k, stride 2) + LayerNorm + GELU as one product
                    k = 3 if i <= 4 else 2
                    add(B * t[i], 512, k * 512, rpb=t[i], flags=LN | s3)
                    add(B * t[i], 512, k * 512, rpb=t[i], flags=s3)  # (fuse_conv_ln = 0)
                M = B * T
                add(M, 1024, 512, flags=s3)               # feature projection
                add(M, 64, 64 * 128, rpb=T, kchunk=64, groups=16, flags=s3)  # positional conv as a chunked-K grouped product
                add(M, 3072, 1024, flags=s3)              # QKV
                add(M, 1024, 1024, flags=s3)              # attention out-projection
                add(M, 4096, 1024, flags=s3)              # FC1 (GELU)
                add(M, 1024, 4096, flags=s3)              # FC2
                add(M, 144, 1024, flags=s3)               # student: trunk -> Conformer tokens
                add(M, 128, 1024, flags=s3 | ACT)         # teacher: trunk -> AASIST (selu)
                for N, K, fl in ((576, 192, ACT), (144, 576, 0), (432, 192, 0), (144, 192, 0), (576, 192, 0), (144, 320, 0)):
                    add(M + B, N, K, flags=s3 | fl)       # Conformer head, one kernel per op (fuse_conformer = 0); + class token
                add(M, 1024, 1024, flags=s3 | NO_DEEP)
                add(M, 1024, 4096, flags=s3 | NO_DEEP)
    for M in (1, 64, 128, 129, 153, 343, 1000, 2048, 3189, 3584, 3589, 6144, 6145, 8192, 10240, 12288, 12741, 16384, 25472, 40000, 65536, 100000):
        for N in (64, 128, 192, 256, 320, 512, 1024, 2048, 3072, 4096):
            for K in (128, 1024):
                add(M, N, K)
                add(M, N, K, flags=S3)
    for M in range(8000, 14001, 500):
        for N in (1024, 3072, 4096):
            add(M, N, 1024)
    for tiles in (255, 256, 257, 300, 352, 353, 512, 600, 800, 801, 3200):  # conv layers around the remainder split
        for rows in (tiles * 128, tiles * 128 - 64, tiles * 128 - 100):
            add(rows, 512, 1536, flags=LN)
            add(rows, 512, 1024, flags=LN)
    return out


def main():
    what = sys.argv[1] if len(sys.argv) > 1 else "shapes"
    if what == "shapes":
        for s in shapes():
            print(*s)
        return
    from afx._lib import check, lib
    obj = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    out = (C.c_int * 8)()
    for s in shapes():
        check(lib().afx_gemm_plan(*s, obj, out))
        print(*s, "", *list(out)[:7])


if __name__ == "__main__":
    main()
