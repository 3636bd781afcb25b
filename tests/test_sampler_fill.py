"""m3d_draw_samples (Mt19937Mod::fill, m3d_mt19937.hpp) against a scalar restatement of the reference's sampler written here:
`rng() % size` on a std::mt19937 seeded with one word, drawn word by word, a repeated index drawn again (utils.h:71-97).

The library accepts the samples that lie inside one 624-word block as a run when none of them holds a repeat and goes through
its scalar code from the first repeat or block edge on; tiny point counts make repeats common, so the two paths alternate, and
huge ones never leave the run path.  The table and the stream consumed must be the scalar ones in every case."""
import numpy as np
import pytest

M_OF_KIND = {0: 3, 1: 4, 2: 2}


class ScalarMt19937:
    """std::mt19937: init_genrand seeding, the 624-word twist, the tempering -- one 32-bit word per next()"""

    def __init__(self, seed):
        mt = [0] * 624
        mt[0] = seed & 0xFFFFFFFF
        for i in range(1, 624):
            mt[i] = (1812433253 * (mt[i - 1] ^ (mt[i - 1] >> 30)) + i) & 0xFFFFFFFF
        self.mt = mt
        self.block = []
        self.pos = 624
        self.words = 0   # outputs consumed so far

    def _twist(self):
        mt = self.mt
        for i in range(624):
            y = (mt[i] & 0x80000000) | (mt[(i + 1) % 624] & 0x7FFFFFFF)
            mt[i] = mt[(i + 397) % 624] ^ (y >> 1) ^ (0x9908B0DF if y & 1 else 0)
        y = np.array(mt, dtype=np.uint64)
        y ^= y >> np.uint64(11)
        y ^= (y << np.uint64(7)) & np.uint64(0x9D2C5680)
        y ^= (y << np.uint64(15)) & np.uint64(0xEFC60000)
        y ^= y >> np.uint64(18)
        self.block = [int(v) for v in y]
        self.pos = 0

    def next(self):
        if self.pos == 624:
            self._twist()
        v = self.block[self.pos]
        self.pos += 1
        self.words += 1
        return v


def scalar_table(n_points, m, n_hyp, seed):
    """-> (table, number of samples that drew at least one word again, words consumed)"""
    g = ScalarMt19937(seed)
    out = np.zeros((n_hyp, m), dtype=np.uint32)
    redrawn = 0
    for h in range(n_hyp):
        s = []
        again = False
        while len(s) < m:
            v = g.next() % n_points
            if v in s:
                again = True
            else:
                s.append(v)
        out[h] = s
        redrawn += again
    return out, redrawn, g.words


def test_restatement_is_the_oracle_sampler(orc):
    for n, m, H, seed in ((5, 3, 700, 1234), (1000, 4, 700, 99), (10**6, 2, 700, 7), (2**32 - 1, 3, 700, 5)):
        t, _, _ = scalar_table(n, m, H, seed)
        assert np.array_equal(t.astype(np.uint64), orc.draw_samples(n, m, H, seed)), (n, m)


# table lengths around the ends of the 624-word blocks (a block holds 208 planes' / 156 spheres' / 312 cylinders' samples when
# nothing is drawn again) and longer ones that cross several blocks
LENGTHS = {0: (1, 207, 208, 209, 416, 417, 1500), 1: (1, 155, 156, 157, 312, 313, 1500), 2: (1, 311, 312, 313, 624, 625, 1500)}
SEEDS = (0, 1, 20240229, 2**32 - 1)


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("n_points", [3, 4, 5, 7, 624, 1000, 1_000_000, 2**32 - 1])
def test_fill_is_the_scalar_stream(capi, kind, n_points):
    m = M_OF_KIND[kind]
    if n_points < m:
        with pytest.raises(capi.M3DError):
            capi.draw_samples(n_points, kind, 10, 1)
        return
    total_redrawn = 0
    for seed in SEEDS:
        full, redrawn_full, words = scalar_table(n_points, m, max(LENGTHS[kind]), seed)
        for H in LENGTHS[kind]:
            a = capi.draw_samples(n_points, kind, H, seed)
            assert a.dtype == np.uint32 and a.shape == (H, m)
            # (a table is a prefix of the longer one: the same stream)
            assert np.array_equal(a, full[:H]), (kind, n_points, seed, H)
        total_redrawn += redrawn_full
        # the long table: what the restatement says about its own run -- words consumed = m per sample + the words drawn again
        assert words >= m * len(full) and (words > m * len(full)) == (redrawn_full > 0)
    if n_points <= 1000:
        # repeats are common: the fall-back and the run path alternate (624 points: one plane sample in 200 holds a repeat)
        assert total_redrawn > 0
    else:
        # none in 4 x 1500 samples (a repeat among four draws from a million points: 6e-6 per sample): the run path only
        assert total_redrawn == 0


def test_stream_position_carries_over_between_tables(capi):
    """a sampler object fills its tables window by window (the chunks of a fit): the windows of any lengths are the one table"""
    n, kind, seed = 6, 0, 77
    full, redrawn, _ = scalar_table(n, 3, 2000, seed)
    assert redrawn > 0
    s = capi.Sampler(n, kind, seed)
    try:
        for upto in (1, 2, 50, 207, 208, 700, 701, 2000):
            got = np.array(s.table(upto), copy=True)
            assert np.array_equal(got, full[:upto]), upto
    finally:
        s.close()
