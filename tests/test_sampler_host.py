"""The sampler's hash (csrc/dpg_sha1.h, the one function the device kernel
calls) compiled for the CPU in a stand-alone program and compared with
hashlib.sha1 over repr(key) on the full key set (no GPU needed)."""
import hashlib
import os
import shutil
import subprocess

from tests import sampler_keys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pipelinedp_amd", "csrc")

MAIN = r"""
#include <cinttypes>
#include <cstdio>
#include "dpg_sha1.h"
int main() {
    long long k;
    while (std::scanf("%lld", &k) == 1)
        std::printf("%" PRIu64 "\n", dpg::sha1_key_hash((int64_t)k));
    return 0;
}
"""


def test_host_build_of_the_hash_equals_sha1(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed (test_native_abi.py needs gcc likewise)"
    src = tmp_path / "sha1_main.cpp"
    src.write_text(MAIN)
    exe = tmp_path / "sha1_main"
    subprocess.run([cxx, "-O2", "-std=c++17", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    keys = sampler_keys.edge_keys() + sampler_keys.random_keys() + list(range(10_000))
    out = subprocess.run([str(exe)], input="\n".join(map(str, keys)), capture_output=True,
                         text=True, check=True)
    got = [int(x) for x in out.stdout.split()]
    want = [int(hashlib.sha1(repr(k).encode()).hexdigest()[:16], 16) for k in keys]
    assert len(got) == len(want)
    bad = [(k, g, w) for k, g, w in zip(keys, got, want) if g != w]
    assert not bad, bad[:5]
