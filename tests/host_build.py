"""How the host tests build their shims: one g++ line for tests/host_*_shim.cpp against the product's headers."""
import ctypes as C
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_shim(tmp_path_factory, source, fast=False, openmp=False):
    """tests/<source> -> a shared library in a fresh temp dir, loaded.  ``fast``: -O3 -march=native instead of -O2 (the
    scalar NN_11 references); -ffp-contract=off always, so that every sum rounds as written."""
    stem = os.path.splitext(source)[0]
    out = tmp_path_factory.mktemp(stem) / f"lib{stem}.so"
    opt = ["-O3", "-march=native"] if fast else ["-O2"]
    subprocess.check_call(["g++", *opt, "-std=c++17", "-ffp-contract=off", *(["-fopenmp"] if openmp else []), "-fPIC", "-shared",
                           "-I", os.path.join(ROOT, "toric-rl-decoder_amd", "csrc"), os.path.join(ROOT, "tests", source),
                           "-o", str(out)])
    return C.CDLL(str(out))
