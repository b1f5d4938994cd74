"""svc::pack_rows (stereovision_amd/csrc/sv_pack.h), the row packing of every host-buffer entry
point, in a stand-alone program built with the host compiler's address and undefined-behaviour
sanitizers: contiguous and padded strides, source and destination sized exactly, the packed
bytes and a canary after the destination checked.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stereovision_amd", "csrc")

MAIN = r"""
#include "sv_pack.h"
#include <algorithm>
#include <cstdio>
#include <vector>

static int run(int H, size_t row, size_t stride) {
    // the source ends with its last row: the pad after it is not the packer's to read
    std::vector<uint8_t> src((size_t)(H - 1) * stride + row);
    for (size_t i = 0; i < src.size(); ++i) src[i] = (uint8_t)(i * 131 + (i >> 8) + 7);
    const size_t n = (size_t)H * row, guard = 16;
    std::vector<uint8_t> dst(n + guard, 0xA5);
    svc::pack_rows(dst.data(), src.data(), H, row, stride);
    for (int y = 0; y < H; ++y)
        for (size_t x = 0; x < row; ++x)
            if (dst[y * row + x] != src[y * stride + x]) {
                std::printf("FAIL H=%d row=%zu stride=%zu: byte (%d, %zu)\n", H, row, stride, y, x);
                return 1;
            }
    for (size_t i = n; i < n + guard; ++i)
        if (dst[i] != 0xA5) {
            std::printf("FAIL H=%d row=%zu stride=%zu: canary byte %zu\n", H, row, stride, i - n);
            return 1;
        }
    uint8_t* exact = new uint8_t[n];   // sized exactly: the sanitizer traps any write past it
    svc::pack_rows(exact, src.data(), H, row, stride);
    const bool same = std::equal(exact, exact + n, dst.begin());
    delete[] exact;
    if (!same) {
        std::printf("FAIL H=%d row=%zu stride=%zu: exact-size destination differs\n", H, row, stride);
        return 1;
    }
    return 0;
}

int main() {
    int bad = run(1, 1, 1) + run(7, 13, 13) + run(7, 13, 14) + run(5, 3 * 11, 3 * 11 + 13);
    std::printf(bad ? "FAILED\n" : "PASS\n");
    return bad ? 1 : 0;
}
"""


def test_pack_rows_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("g++ not available")
    src = tmp_path / "pack_rows_main.cpp"
    src.write_text(MAIN)
    exe = tmp_path / "pack_rows_main"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, str(src),
                        "-o", str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and r.stdout.strip().endswith("PASS"), r.stdout + r.stderr
