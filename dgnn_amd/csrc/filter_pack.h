// The filter product of the fp16 two-part form in TWO v_mfma_f32_16x16x32_f16 per channel block: the slot map, written once.
//
// phi = [A | 1] . [We^T ; be]: K = 21 real indices (20 edge attributes and the constant 1 that multiplies the bias row).  With A = ah + al and
// B = bh + bl (fused_common.h: split2h under power-of-two scales) the product keeps ah.bh (21 terms), ah.bl (21) and al.bh (20: the lo part of the
// constant slot 1.0 * sA is exactly zero, sA being a power of two) and drops al.bl: 62 terms.  As three products of 32 K-slots each (al.bh, ah.bl, ah.bh)
// 34 of 96 slots multiplied zeros.  Two products hold 64 slots: the map below says which term sits in which.
//
// A product has four lane groups g = lane >> 4 of 8 K-slots each (slot s of group g = element s of the lane's operand register).  M2 is issued first,
// M1 on top of it (small terms first, as in every product of this form: every hi.hi term is in M1).  A lane of the A side holds EIGHT values of its
// edge, from two 16-byte loads, and every slot of the lane is a part of one of them -- no value crosses lanes, none is loaded twice by a lane:
//   group   the lane's eight values          M1 = the hi words of the eight, times              M2 (words w0 .. w3)
//   g0      a0..7                            bh0..7                                             l0,1.bh  l2,3.bh    h2,3.bl    h0,1.bl
//   g1      a8..15                           bh8..15                                            h12,13.bl h14,15.bl l12,13.bh  l14,15.bh
//   g2      a16 a17 a18 a19 | 1 0 | a16 a17  bh16..19, (bh20, -), bl16,17                       l16,17.bh l18,19.bh h18,19.bl  (h20, -).bl
//   g3      a4..11                           bl4..11                                            l4,5.bh  l6,7.bh    l8,9.bh    l10,11.bh
// Attributes 0-3, 12-15 and 16-20 have all their terms in the group that loaded them; 4-7 and 8-11 have hi.lo and lo.hi in g3, which loads the middle
// of the row.  Whole 32-bit words everywhere: a word is two neighbouring K indices (2 i, 2 i + 1) of ONE part -- (h20, 0) for the constant, whose odd
// half is the one unused slot of each product -- so a lane picks words of what split2h gave it (ph, pl) and permutes no bytes:
//   w0 = g1 ? ph[2] : pl[0]    w1 = g1 ? ph[3] : pl[1]    w2 = (g & 1) ? pl[2] : ph[1]    w3 = (g & 1) ? pl[3] : (g0 ? ph[0] : ph[2])
//
// No device code here: tests/test_filter_pack_cpu.py compiles a host program against this header.
#pragma once

namespace filter_pack {

constexpr int FE = 20;            // edge attributes; K index FE = the constant 1 (A side) / the bias (B side)
constexpr int NK = FE + 1;
constexpr int NTERMS = 3 * NK - 1;

enum Part : signed char { NONE = 0, HI = 1, LO = 2 };
struct Slot {
    signed char a, b;   // part of the scaled attribute row / of [We | be] . sWe in this slot (NONE: unused, zero on the A side)
    signed char k;      // K index of both (-1: unused)
};
constexpr int M2 = 0, M1 = 1;     // issue order

// eight slots from K index k0 on, parts (a, b)
#define FP_ROW8(a, b, k0)                                                                                                              \
    {Slot{a, b, k0}, Slot{a, b, k0 + 1}, Slot{a, b, k0 + 2}, Slot{a, b, k0 + 3}, Slot{a, b, k0 + 4}, Slot{a, b, k0 + 5}, Slot{a, b, k0 + 6}, \
     Slot{a, b, k0 + 7}}
#define FP_W(a, b, k0) Slot{a, b, k0}, Slot{a, b, k0 + 1}
#define FP_WC(b) Slot{HI, b, FE}, Slot{NONE, NONE, -1}     // the constant's word
constexpr Slot MAP[2][4][8] = {
    // M2
    {{FP_W(LO, HI, 0), FP_W(LO, HI, 2), FP_W(HI, LO, 2), FP_W(HI, LO, 0)},
     {FP_W(HI, LO, 12), FP_W(HI, LO, 14), FP_W(LO, HI, 12), FP_W(LO, HI, 14)},
     {FP_W(LO, HI, 16), FP_W(LO, HI, 18), FP_W(HI, LO, 18), FP_WC(LO)},
     {FP_W(LO, HI, 4), FP_W(LO, HI, 6), FP_W(LO, HI, 8), FP_W(LO, HI, 10)}},
    // M1
    {FP_ROW8(HI, HI, 0), FP_ROW8(HI, HI, 8),
     {FP_W(HI, HI, 16), FP_W(HI, HI, 18), FP_WC(HI), FP_W(HI, LO, 16)},
     FP_ROW8(HI, LO, 4)},
};
#undef FP_W
#undef FP_WC
#undef FP_ROW8

// ---- the properties the kernels rely on (checked here at compile time, and again by the host program of the test)
// every one of the 62 terms exactly once, nothing else
constexpr int count_term(int a, int b, int k) {
    int n = 0;
    for (int m = 0; m < 2; ++m)
        for (int g = 0; g < 4; ++g)
            for (int s = 0; s < 8; ++s) n += MAP[m][g][s].a == a && MAP[m][g][s].b == b && MAP[m][g][s].k == k;
    return n;
}
constexpr bool terms_once() {
    int used = 0;
    for (int k = 0; k < NK; ++k) {
        if (count_term(HI, HI, k) != 1 || count_term(HI, LO, k) != 1) return false;
        if (count_term(LO, HI, k) != (k < FE ? 1 : 0) || count_term(LO, LO, k) != 0) return false;
    }
    for (int m = 0; m < 2; ++m)
        for (int g = 0; g < 4; ++g)
            for (int s = 0; s < 8; ++s) {
                const Slot t = MAP[m][g][s];
                if (t.k >= 0) {
                    if (t.k >= NK || t.a == NONE || t.b == NONE) return false;
                    ++used;
                } else if (t.a != NONE || t.b != NONE) {
                    return false;
                }
            }
    return used == NTERMS;
}
// a 32-bit word = slots (2 d, 2 d + 1): K indices (2 i, 2 i + 1) of one part on each side; the constant's word is (k = 20, unused)
constexpr bool words_whole() {
    for (int m = 0; m < 2; ++m)
        for (int g = 0; g < 4; ++g)
            for (int d = 0; d < 4; ++d) {
                const Slot e = MAP[m][g][2 * d], o = MAP[m][g][2 * d + 1];
                if (e.k < 0 || (e.k & 1)) return false;
                if (e.k == FE ? o.k != -1 : (o.k != e.k + 1 || o.a != e.a || o.b != e.b)) return false;
            }
    return true;
}
// the K index of value i of the eight a lane of group g holds (-1: the zero behind the constant)
constexpr int LANE_K[4][8] = {{0, 1, 2, 3, 4, 5, 6, 7}, {8, 9, 10, 11, 12, 13, 14, 15}, {16, 17, 18, 19, FE, -1, 16, 17}, {4, 5, 6, 7, 8, 9, 10, 11}};
// M1's A side is the hi words of the lane's eight values, in their order
constexpr bool m1_is_hi() {
    for (int g = 0; g < 4; ++g)
        for (int s = 0; s < 8; ++s)
            if (MAP[M1][g][s].k != LANE_K[g][s] || (MAP[M1][g][s].k >= 0 && MAP[M1][g][s].a != HI)) return false;
    return true;
}
// every word of M2's A side is a word (hi or lo) of the lane's eight values: nothing crosses lanes
constexpr bool m2_is_own() {
    for (int g = 0; g < 4; ++g)
        for (int d = 0; d < 4; ++d) {
            bool found = false;
            for (int i = 0; i < 4; ++i) found = found || LANE_K[g][2 * i] == MAP[M2][g][2 * d].k;
            if (!found) return false;
        }
    return true;
}
// word d of group g in product m is, on the A side, part `a` from K index k on (what a kernel's hand-written selects assert)
constexpr bool a_word(int m, int g, int d, int a, int k) { return MAP[m][g][2 * d].a == a && MAP[m][g][2 * d].k == k; }
static_assert(terms_once(), "62 terms, each once");
static_assert(words_whole(), "whole words of one part");
static_assert(m1_is_hi(), "M1 = the hi words of the lane's eight values");
static_assert(m2_is_own(), "M2 = words of the lane's eight values");

}  // namespace filter_pack
