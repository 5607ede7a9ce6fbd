"""Addresses and coverage of the window-sharing three-plane conv GEMM (gemm_win_b3_stream_shared_kernel), checked on the host.

The kernel takes every tile's and every slab row's context -- byte offset, k-tile range, stored rows -- from three functions of
rstnet_amd/csrc/b3_common.h and forms its load offsets with a fourth.  A host-only program around the same functions enumerates every
tile of the shapes below (the GPU test's, the codec's, and a batch stride larger than an utterance) and asserts:
 (a) every byte offset the k loop can form -- k-tiles inside and outside a row's range, parked rows, the request stream running past the
     group at the end of a run -- lies inside [0, ((B - 1) * x_bstride + T_in * C) * 4 - 16];
 (b) every output row of every utterance is stored by exactly one tile;
 (c) tap h of a stored row reads, k-tile by k-tile, what the convolution's window reads: A(b, t, k) = x_b[(t * S - P) * C + k] inside the
     utterance, zero outside.
The buffer loads of the kernel are not range-checked by the hardware, so (a) is what keeps it inside its operand."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rstnet_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "b3_common.h"

int main(int argc, char** argv) {
    if (argc != 8) return 2;
    const int R = atoi(argv[1]), B = atoi(argv[2]), T_in = atoi(argv[3]), T_out = atoi(argv[4]), C = atoi(argv[5]), S = atoi(argv[6]);
    const long x_bstride = atol(argv[7]);
    const int G = S * C, TC = T_in * C, P = (R - 1) * S, nkg = G / 16;
    const long last = ((long)(B - 1) * x_bstride + (long)T_in * C) * 4 - 16;
    const int tiles_m = B * b3_shared_tiles_per_utt(T_out, R);
    std::vector<int> stored((size_t)B * T_out, 0);
    long bad_offset = 0, bad_window = 0, bad_tile = 0, offsets = 0;
    for (int mt = 0; mt < tiles_m; ++mt) {
        const B3SharedTile t = b3_shared_tile(mt, R, T_out);
        if (t.b < 0 || t.b >= B || t.t0 < 0 || t.t0 >= T_out || t.m0 != (long)t.b * T_out + t.t0 || t.mlim <= t.m0 ||
            t.mlim - t.m0 > b3_shared_step(R) || t.mlim > (long)(t.b + 1) * T_out) {
            ++bad_tile;
            continue;
        }
        for (long m = t.m0; m < t.mlim; ++m) ++stored[(size_t)m];
        for (int r = 0; r < B3_SH_ROWS; ++r)
            for (int lk = 0; lk < 16; lk += 4) {
                const B3SharedRow row = b3_shared_row(t, r, R, G, TC, x_bstride, lk);
                // the request stream: k-tiles 0 .. nkg - 1 of the group, and up to four past it when the run ends
                for (int kt = 0; kt < nkg + 4; ++kt) {
                    bool ok;
                    const unsigned vo = b3_shared_load_offset(row, kt, ok);
                    ++offsets;
                    if ((long)vo > last || vo % 16 != 0) ++bad_offset;
                }
                // (c) this slab row as tap h of accumulator row i = r - h
                for (int h = 0; h < R; ++h) {
                    const int i = r - h;
                    if (i < 0 || t.m0 + i >= t.mlim) continue;
                    const long f0 = ((long)(t.t0 + i) * S - P) * C + (long)h * G;       // window start of the row + the tap's k range
                    for (int kt = 0; kt < nkg; ++kt) {
                        bool ok;
                        const unsigned vo = b3_shared_load_offset(row, kt, ok);
                        const long f = f0 + kt * 16 + lk;
                        const bool inside = f >= 0 && f + 4 <= TC;
                        if (!inside && (f + 3 >= 0 && f < TC)) ++bad_window;           // a 16-byte piece never straddles the edge
                        if (ok != inside) ++bad_window;
                        if (ok && (long)vo != ((long)t.b * x_bstride + f) * 4) ++bad_window;
                    }
                }
            }
    }
    long not_once = 0;
    for (int v : stored) not_once += v != 1;
    printf("tiles %d offsets %ld bad_tile %ld bad_offset %ld bad_window %ld rows_not_stored_once %ld\n", tiles_m, offsets, bad_tile, bad_offset,
           bad_window, not_once);
    return (bad_tile || bad_offset || bad_window || not_once) ? 1 : 0;
}
"""

# R, B, T_in, T_out (= ceil(T_in / S): conv1d's frame count; T_in for the transposed convs), C, S, x_bstride
SHAPES = [
    (2, 3, 5999, 1500, 16, 4, 5999 * 16),            # strided, partial last group, ragged last tile
    (2, 2, 131075, 32769, 64, 4, 131075 * 64),       # strided, the wide-tile case
    (3, 40, 110, 110, 64, 1, 110 * 64),              # utterances shorter than a tile
    (3, 5, 1016, 1016, 64, 1, 1016 * 64),
    (3, 5, 1017, 1017, 64, 1, 1017 * 64),
    (3, 5, 1008, 1008, 64, 1, 1008 * 64),            # 8 * 126: the row limit exactly on a tile edge
    (3, 5, 1009, 1009, 64, 1, 1009 * 64),
    (2, 5, 1016, 1016, 64, 1, 1016 * 64),            # 8 * 127
    (2, 5, 1017, 1017, 64, 1, 1017 * 64),
    (2, 3, 1500, 1500, 128, 1, 1500 * 128),          # transposed conv, stride 5
    (2, 1, 1, 1, 64, 1, 64),                         # one frame
    (3, 2, 2, 2, 64, 1, 200),                        # batch stride larger than the utterance
    (2, 64, 2000, 250, 512, 8, 2000 * 512),          # codec, batch 64 x 10 s: the deepest strided conv (K = 8192)
    (2, 4, 240000, 60000, 64, 4, 240000 * 64),       # codec: the first strided conv
    (3, 4, 12000, 12000, 256, 1, 12000 * 256),       # codec: a k3 conv
    (2, 64, 250, 250, 1024, 1, 250 * 1024),          # codec: the first transposed conv
]


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    d = tmp_path_factory.mktemp("b3_shared")
    src, exe = os.path.join(d, "b3_shared_ctx.cpp"), os.path.join(d, "b3_shared_ctx")
    with open(src, "w") as f:
        f.write(PROGRAM)
    subprocess.check_call([HIPCC, "-x", "hip", "--offload-host-only", "-O2", "-std=c++17", "-I", CSRC, src, "-o", exe])
    return exe


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "R{}_B{}_T{}_C{}_S{}".format(s[0], s[1], s[2], s[4], s[5]))
def test_shared_tile_addresses_and_coverage(checker, shape):
    R, B, T_in, T_out, C, S, x_bstride = shape
    assert T_out == -(-T_in // S) and (S * C) % 64 == 0
    r = subprocess.run([checker] + [str(v) for v in shape], capture_output=True, text=True, timeout=300)
    print(r.stdout.strip())
    assert r.returncode == 0, r.stdout + r.stderr
