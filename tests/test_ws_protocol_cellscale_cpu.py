"""The decoder stages of the wave-specialised last layer (dgnn_amd/csrc/fused_ws.hip, DEC instantiation) with the per-cell scale, as a model under a
randomised scheduler (the ring hand-off itself: test_ws_protocol_cpu.py).

Per tile t a consumer runs, in its iteration `it`: C(it - 4) (consumer 0), the product of tile it - 1 with A1(it - 1) behind it, A2(it - 2), B(it - 3)
(or the producers run B(it - 3) in their iteration `it`).  A1 folds the consumer's exponents into the tile's tagged words cmax[t % NB] and counts into
ccnt[t & 1]; A2 waits for ccnt and yfree, reads the words, parks its channels in ytile[t & 1], counts into ycnt[t & 1]; B and C as before.  A tagged
word holds the LATEST tile written to it, so a reader must find its own tile's tag there: the model raises when an A1 of a later tile got in first.
The kernel ships NB = 4 buffers of words and no wait in A1; NB = 2 is the variant the header comment of the kernel rules out."""
import random

import pytest

NP = NC = 8


class Violation(Exception):
    pass


def simulate(n_tiles, seed, nb_cmax=4, b_on_consumers=lambda t: t % 4 != 3, ring=2, steps=400000):
    rng = random.Random(seed)
    ready, done = [0] * ring, [0] * ring
    ccnt, ycnt, yfree, lcnt = ([0, 0] for _ in range(4))
    cmax = [[None] * NC for _ in range(nb_cmax)]              # (tile) of consumer c's latest contribution to the buffer's words
    ytile = [[None] * NC for _ in range(2)]
    plog = [[None] * 8 for _ in range(2)]
    logits = {}

    def wait(cond):
        while not cond():
            yield

    def stage_b(t, job):
        yield from wait(lambda: ycnt[t & 1] >= 8 * (t // 2 + 1))
        yield
        for c in range(NC):
            if ytile[t & 1][c] != t:
                raise Violation("stage B of tile %d, job %d: consumer %d's channels in the buffer are tile %s's" % (t, job, c, ytile[t & 1][c]))
        yield
        yfree[t & 1] += 1
        yield
        plog[t & 1][job] = t
        yield
        lcnt[t & 1] += 1

    def producer(p):
        for it in range(n_tiles + 3):
            if it >= 3 and not b_on_consumers(it - 3):
                yield from stage_b(it - 3, p)
            if it >= n_tiles:
                continue
            sl = it % ring
            yield
            yield from wait(lambda: done[sl] >= NC * (it // ring))
            yield
            ready[sl] += 1

    def consumer(c):
        for it in range(1, n_tiles + 3 + 1):
            if c == 0 and it >= 4:                             # C(it - 4)
                t = it - 4
                yield from wait(lambda: lcnt[t & 1] >= 8 * (t // 2 + 1))
                yield
                for j in range(8):
                    if plog[t & 1][j] != t:
                        raise Violation("stage C of tile %d: job %d's partial logits in the buffer are tile %s's" % (t, j, plog[t & 1][j]))
                logits[t] = True
            if it <= n_tiles:                                  # product and A1 of tile it - 1
                t = it - 1
                sl = t % ring
                yield from wait(lambda: ready[sl] >= NP * (t // ring + 1))
                yield
                done[sl] += 1
                yield
                cmax[t % nb_cmax][c] = t
                yield
                ccnt[t & 1] += 1
            if 2 <= it <= n_tiles + 1:                         # A2(it - 2)
                t = it - 2
                yield from wait(lambda: ccnt[t & 1] >= 8 * (t // 2 + 1))
                yield from wait(lambda: yfree[t & 1] >= 8 * (t // 2))
                yield
                for c2 in range(NC):
                    if cmax[t % nb_cmax][c2] != t:
                        raise Violation("stage A2 of tile %d, consumer %d: consumer %d's exponent in the word is tile %s's" % (t, c, c2, cmax[t % nb_cmax][c2]))
                yield
                ytile[t & 1][c] = t
                yield
                ycnt[t & 1] += 1
            if 3 <= it <= n_tiles + 2 and b_on_consumers(it - 3):
                yield from stage_b(it - 3, c)

    actors = [producer(p) for p in range(NP)] + [consumer(c) for c in range(NC)]
    live = list(range(len(actors)))
    n = 0
    while live:
        n += 1
        if n > steps:
            raise AssertionError("no progress: deadlock in the model")
        k = rng.choice(live)
        for _ in range(rng.choice((1, 1, 2, 5, 30, 200))):
            try:
                next(actors[k])
            except StopIteration:
                live.remove(k)
                break
    if sorted(logits) != list(range(n_tiles)):
        raise Violation("logits stored for tiles %s of %d" % (sorted(logits), n_tiles))
    return n


@pytest.mark.parametrize("split", ["producers", "even", "three_of_four", "consumers"])
def test_four_stage_decoder_survives_random_schedules_and_drains(split):
    rule = {"producers": lambda t: False, "even": lambda t: t % 2 == 0, "three_of_four": lambda t: t % 4 != 3, "consumers": lambda t: True}[split]
    for seed in range(100):
        for n_tiles in (0, 1, 2, 3, 5, 11):
            simulate(n_tiles, seed, b_on_consumers=rule)


def test_two_buffers_of_exponent_words_are_caught():
    """a consumer one iteration ahead of the slowest writes tile t + 2's exponents over words the slowest has not read for tile t"""
    hit = None
    for seed in range(400):
        try:
            simulate(8, seed, nb_cmax=2, b_on_consumers=lambda t: False)
        except Violation as e:
            hit = str(e)
            break
    assert hit is not None and "stage A2" in hit, hit
