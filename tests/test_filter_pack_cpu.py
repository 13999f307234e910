"""The slot map of the two-product filter form (dgnn_amd/csrc/filter_pack.h), checked by a stand-alone host program (no GPU, nothing loaded into Python).

The fused fp16 two-part kernels pack the 62 real terms of phi = [A | 1] . [We^T ; be] (21 hi.hi, 21 hi.lo, 20 lo.hi) into the 64 K-slots of two
v_mfma_f32_16x16x32_f16.  The kernels fill the B fragments from the map and assert their A-side selects against it, so what has to hold is the map:
every term exactly once, the A and the B slot of a term on the same k, whole 32-bit words of one part, zeros on the A side of the unused slots.  The
program walks the map AS AN MFMA WOULD: it builds both operands of both products for a probe row and a probe weight row whose every (part, k) carries its
own prime, multiplies slot by slot, and compares the multiset of products with the 62 expected ones.  Built with the address and undefined-behaviour
sanitizers where the host compiler has them."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")

PROGRAM = r"""
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>

#include "filter_pack.h"

using namespace filter_pack;

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("FAILED line %d: %s\n", __LINE__, #c);          \
            return 1;                                                   \
        }                                                               \
    } while (0)

int main() {
    // (part, k) -> a value of its own: distinct primes, so a product names its two factors
    std::vector<long> primes;
    for (long n = 2; primes.size() < 4 * NK; ++n) {
        bool p = true;
        for (long d = 2; d * d <= n; ++d) p = p && n % d != 0;
        if (p) primes.push_back(n);
    }
    auto aval = [&](int part, int k) -> long { return part == NONE ? 0 : (part == LO && k == FE ? 0 : primes[(part - 1) * NK + k]); };   // lo of the constant slot is 0
    auto bval = [&](int part, int k) -> long { return part == NONE ? 0 : primes[(2 + part - 1) * NK + k]; };

    std::map<long, int> got;
    int used = 0, unused = 0;
    for (int m = 0; m < 2; ++m)
        for (int g = 0; g < 4; ++g)
            for (int s = 0; s < 8; ++s) {
                const Slot t = MAP[m][g][s];
                if (t.k < 0) {
                    // an unused slot: nothing on the A side (the kernels leave zero there: the odd half of the constant's word)
                    CHECK(t.a == NONE && t.b == NONE);
                    CHECK(aval(t.a, 0) == 0);
                    CHECK(s % 2 == 1 && MAP[m][g][s - 1].k == FE);
                    ++unused;
                    continue;
                }
                CHECK(t.k < NK);
                CHECK(t.a == HI || t.a == LO);
                CHECK(t.b == HI || t.b == LO);
                CHECK(!(t.a == LO && t.b == LO));          // lo.lo is the dropped product
                CHECK(!(t.a == LO && t.k == FE));          // the constant has no lo part
                // the A slot and the B slot of this position carry the same k: one Slot has ONE k by construction; the product says which two met
                got[aval(t.a, t.k) * bval(t.b, t.k)] += 1;
                ++used;
            }
    CHECK(used == 62 && unused == 2 && NTERMS == 62);

    std::map<long, int> want;
    for (int k = 0; k < NK; ++k) {
        want[aval(HI, k) * bval(HI, k)] += 1;
        want[aval(HI, k) * bval(LO, k)] += 1;
        if (k < FE) want[aval(LO, k) * bval(HI, k)] += 1;
    }
    CHECK(want.size() == 62);
    CHECK(got == want);                                    // 62 distinct terms, each exactly once
    for (const auto& kv : got) CHECK(kv.second == 1);

    // word pairs: slots (2 d, 2 d + 1) = K indices (2 i, 2 i + 1) of one part on each side; the constant's word is (20, unused)
    for (int m = 0; m < 2; ++m)
        for (int g = 0; g < 4; ++g)
            for (int d = 0; d < 4; ++d) {
                const Slot e = MAP[m][g][2 * d], o = MAP[m][g][2 * d + 1];
                CHECK(e.k >= 0 && e.k % 2 == 0);
                if (e.k == FE) CHECK(o.k == -1);
                else CHECK(o.k == e.k + 1 && o.a == e.a && o.b == e.b);
            }

    // what the kernels' A side assumes.  A lane holds eight values of its edge (two 16-byte loads: attributes from 0 / 8 / 4 on in k-groups 0 / 1 / 3,
    // [16 17 18 19 | 20 - | 16 17] in k-group 2): M1 = their hi words in their order, every word of M2 = a hi or lo word of the same eight
    const int first[4] = {0, 8, 16, 4};
    for (int g = 0; g < 4; ++g)
        for (int s = 0; s < 8; ++s) {
            const int k = g != 2 ? first[g] + s : (s < 4 ? 16 + s : (s == 4 ? FE : (s == 5 ? -1 : 10 + s)));
            CHECK(LANE_K[g][s] == k);
            CHECK(MAP[M1][g][s].k == k);
            if (k >= 0) CHECK(MAP[M1][g][s].a == HI);
            if (s % 2 == 0) {
                bool own = false;
                for (int i = 0; i < 8; i += 2) own = own || LANE_K[g][i] == MAP[M2][g][s].k;
                CHECK(own);
            }
        }
    // small terms first: every hi.hi term sits in the product issued last
    for (int g = 0; g < 4; ++g)
        for (int s = 0; s < 8; ++s) CHECK(!(MAP[M2][g][s].a == HI && MAP[M2][g][s].b == HI));
    CHECK(M2 == 0 && M1 == 1);
    std::printf("filter_pack ok: %d terms, %d unused slots\n", used, unused);
    return 0;
}
"""


def _build(tmp_path, flags):
    src = tmp_path / "filter_pack_check.cpp"
    src.write_text(PROGRAM)
    exe = str(tmp_path / "filter_pack_check")
    r = subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "dgnn_amd", "csrc"), str(src), "-o", exe],
                       capture_output=True, text=True)
    return exe, r


@pytest.mark.skipif(CXX is None, reason="needs a host C++ compiler")
def test_slot_map_holds_every_term_once(tmp_path):
    exe, r = _build(tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if r.returncode != 0:
        exe, r = _build(tmp_path, [])          # a host compiler without the sanitizers' runtime libraries: the same program without them
    assert r.returncode == 0, r.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "filter_pack ok: 62 terms, 2 unused slots" in run.stdout
