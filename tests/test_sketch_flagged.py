"""The seed stage's sketch (a1, MinCount.h:8-179) when some, all or none of a batch's reads hold a non-ACGT byte: the wave kernel lists those reads and the serial
kernel runs over the list alone (and is not launched for an empty one).  Through seed.seed_batch, as tests/test_seed.py goes, against the oracle's minimizers."""
import functools

import numpy as np
import pytest

import oracle_lib as O
from lra_amd import synth

K, W = 15, 10
SPAN = W + K - 1


@functools.lru_cache(maxsize=None)
def _reference():
    genome = synth.make_genome(120000, seed=12, repeat_frac=0.2)
    ik, ip = synth.build_global_index(genome, K, W, 50)
    return genome, ik, ip


def _reads(n, seed, flagged=(), short_flagged=()):
    """n reads of 200-3000 bases off the reference; the reads of `flagged` get non-ACGT bytes, those of `short_flagged` are cut below w + k - 1 and get one."""
    genome = _reference()[0]
    rng = np.random.default_rng(seed)
    out = []
    for r in range(n):
        L = int(rng.integers(200, 3001)); s = int(rng.integers(0, len(genome) - L))
        x = genome[s:s + L].copy()
        m = rng.random(L) < 0.05
        x[m] = synth.BASES[rng.integers(0, 4, int(m.sum()))]
        if r in short_flagged:
            x = x[:int(rng.integers(1, SPAN))].copy(); x[len(x) // 2] = ord("N")
        elif r in flagged:
            kind = r % 4
            if kind == 0: x[int(rng.integers(0, L))] = ord("N")                                   # one N anywhere
            elif kind == 1: x[0] = ord("N"); x[L - 1] = ord("n")                                   # at both ends
            elif kind == 2: x[rng.integers(0, L, 6)] = np.frombuffer(b"NRYKMN", np.uint8)          # scattered, other IUPAC letters too
            else: a = int(rng.integers(0, L - 60)); x[a:a + 50] = ord("N")                         # a run
        out.append(x)
    return out


def _check(ctx, reads, n_flagged):
    from lra_amd import seed
    genome, ik, ip = _reference()
    acgt = np.zeros(256, bool); acgt[list(b"ACGTacgt")] = True
    assert sum(1 for r in reads if not acgt[r].all()) == n_flagged                                 # the batch holds the case it is for
    batch = seed.ReadBatch(ctx, [r.tobytes() for r in reads])
    res = seed.seed_batch(ctx, batch, K, W, 150)
    out = seed.fetch(ctx, res)
    total = 0
    for r, read in enumerate(reads):
        sk, sp = O.sort_minimizers(*O.store_minimizers(read.tobytes(), K, W))
        a, b = int(out["mm_off"][r]), int(out["mm_off"][r + 1])
        assert b - a == len(sk), (r, len(read), b - a, len(sk))
        assert np.array_equal(out["mm_key"][a:b], sk) and np.array_equal(out["mm_pos"][a:b], sp), (r, len(read))
        total += len(sk)
    assert int(out["mm_off"][len(reads)]) == total
    return total


@pytest.fixture(scope="module")
def loaded(ctx):
    from lra_amd import seed
    genome, ik, ip = _reference()
    seed.load_reference(ctx, genome, ik, ip)
    return ctx


@pytest.mark.gpu
def test_hip_sketch_no_read_flagged(loaded):
    assert _check(loaded, _reads(70, 1), 0) > 5000
    assert _check(loaded, _reads(3, 2), 0) > 100


@pytest.mark.gpu
def test_hip_sketch_every_read_flagged(loaded):
    assert _check(loaded, _reads(70, 3, flagged=range(70)), 70) > 5000
    assert _check(loaded, _reads(3, 4, flagged=range(3)), 3) > 100


@pytest.mark.gpu
def test_hip_sketch_flagged_at_block_boundaries(loaded):
    """Reads 0, 63, 64 (where the lane-per-read kernel's workgroups over all reads met) and the last one; one flagged read shorter than w + k - 1."""
    assert _check(loaded, _reads(70, 5, flagged=(0, 63, 64, 69)), 4) > 5000
    assert _check(loaded, _reads(66, 6, flagged=(0, 63, 64, 65), short_flagged=(17,)), 5) > 5000
    assert _check(loaded, _reads(65, 7, flagged=(64,), short_flagged=(0, 63)), 3) > 5000


@pytest.mark.gpu
def test_hip_sketch_with_n_then_without_on_one_context(loaded):
    """One batch after another: a list or a count left over from the batch before would show in the next."""
    with_n = _reads(40, 8, flagged=(1, 5, 39)); without = _reads(40, 9); many = _reads(12, 10, flagged=range(12))
    for reads, nf in ((with_n, 3), (without, 0), (many, 12), (without, 0), (with_n, 3)):
        assert _check(loaded, reads, nf) > 1000
