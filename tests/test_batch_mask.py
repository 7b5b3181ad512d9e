"""N-masked full-length copies of resident records (Device.batch_mask -> ntl_batch_mask, csrc/mask_kernels.h) and Batch.download_n
(ntl_batch_download_n) -- under the SIMT mock and on the GPU, the same checks.
  a. crafted records: batch_mask(...).download_n() == the upper-cased, N-substituted Python string, and the sketch of the masked batch
     at (k, w) = (20, 10) and (15, 5) == the sketch of Device.batch over the Python-masked ASCII, record for record
  b. 300 random (source, range) draws over sources with random N runs: the same two comparisons
  c. NTL_EINVAL with a message for a source number, a reversed range and a range beyond the record; a masked batch destroyed right
     after a sketch was queued on it"""
import functools

import numpy as np
import pytest

from ntlink_amd import capi

KW = ((20, 10), (15, 5))
ACGT = np.frombuffer(b"ACGT", np.uint8)
VALID = frozenset(b"ACGTacgt")
SMALL = (0, 1, 15, 16, 17, 19, 20, 21, 31, 32, 33)


def rand(rng, n):
    return ACGT[rng.integers(0, 4, n)].tobytes()


def masked(seq, lo, hi):
    """what print_masked_sequences writes for the range, as a batch holds it: upper case, N for every other byte"""
    body = bytes(c if c in VALID else 78 for c in seq[lo:hi]).upper()
    return b"N" * lo + body + b"N" * (len(seq) - hi)


@functools.lru_cache(maxsize=None)
def crafted():
    """(sources, [(source number, keep_lo, keep_hi)])"""
    rng = np.random.default_rng(5)
    sources = [rand(rng, 37)]  # odd: no later source starts on a word boundary by accident of the lengths alone
    cases = [(0, 0, 37), (0, 1, 36)]
    for n in SMALL:
        s = len(sources)
        sources.append(rand(rng, n))
        cases += [(s, 0, n), (s, 0, 0), (s, n, n), (s, n // 2, n // 2)]
        if n >= 2:
            cases += [(s, 1, n), (s, 0, n - 1)]
    long = len(sources)
    sources.append(rand(rng, 9000))  # more than one strip of 4096 k-mers
    cases += [(long, 0, 9000), (long, 100, 8300), (long, 4090, 4100), (long, 4000, 8999)]  # starts and ends in different strips
    cases += [(long, 16 * 5 + a, 16 * 40 + b) for a in (0, 1, 15) for b in (0, 1, 15)]
    cases += [(long, 1000, 1000 + n) for n in (10, 14, 15, 19, 20, 29, 30)]        # shorter than k, exactly k, k + w - 1, for both (k, w)
    cases += [(long, 8190 - n, 8190) for n in (15, 19, 20, 29)]
    multi = len(sources)
    #                 run [0, 100)      N x 7     run [107, 167) lower    R     run [168, 368)     N x 30     run [398, 548)
    sources.append(rand(rng, 100) + b"N" * 7 + rand(rng, 60).lower() + b"R" + rand(rng, 200) + b"N" * 30 + rand(rng, 150))
    cases += [(multi, 0, 548), (multi, 50, 450),                       # whole; three runs and more, clipped at both ends
              (multi, 99, 108), (multi, 107, 167), (multi, 166, 169),  # ends on the last / first base of a run
              (multi, 108, 166), (multi, 100, 107), (multi, 101, 106), (multi, 370, 390),  # one base inside a run; inside N stretches
              (multi, 167, 168), (multi, 150, 420), (multi, 398, 548), (multi, 397, 399)]
    mixed = len(sources)
    sources.append(b"nnnn" + rand(rng, 45) + b"YK" + rand(rng, 19) + b"N" + rand(rng, 20) + b"n" + rand(rng, 21).lower() + b"NN")
    cases += [(mixed, 0, len(sources[mixed])), (mixed, 4, 49), (mixed, 3, 50), (mixed, 51, 112), (mixed, 60, 100)]
    assert sum(1 for c in cases if c[0] == long) >= 4
    return sources, cases


@functools.lru_cache(maxsize=None)
def random_cases(seed=77, n=300):
    rng = np.random.default_rng(seed)
    sources = []
    for _ in range(14):
        seq = bytearray(rand(rng, int(rng.integers(1, 1500))))
        for _run in range(int(rng.integers(0, 6))):
            a = int(rng.integers(0, len(seq)))
            b = min(len(seq), a + int(rng.integers(1, 40)))
            seq[a:b] = b"N" * (b - a)
        sources.append(bytes(seq))
    cases = []
    for _ in range(n):
        s = int(rng.integers(0, len(sources)))
        lo, hi = sorted(rng.integers(0, len(sources[s]) + 1, 2).tolist())
        cases.append((s, lo, hi))
    return sources, cases


@functools.lru_cache(maxsize=None)
def reference_records(which):
    """the Python-masked ASCII of every case: computed once, shared"""
    sources, cases = crafted() if which == "crafted" else random_cases()
    return [masked(sources[s], lo, hi) for s, lo, hi in cases]


def compare(dev, src_batch, cases, want):
    sq, lo, hi = (np.array(col, np.uint32) for col in zip(*cases)) if cases else (np.zeros(0, np.uint32),) * 3
    with dev.batch_mask(src_batch, sq, lo, hi) as mb, dev.batch(want) as ref:
        assert mb.nseq == len(cases) and mb.bases == sum(len(w) for w in want)
        buf, off = mb.download_n()
        assert off.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
        raw = buf.tobytes()
        for i, w in enumerate(want):
            got = raw[int(off[i]):int(off[i + 1])]
            assert got == w, f"record {i} {cases[i]}: {got[:80]!r}..., the masked string is {w[:80]!r}..."
        assert ref.download_n()[0].tobytes() == b"".join(want)
        for k, w in KW:
            with dev.sketch(mb, k, w) as a, dev.sketch(ref, k, w) as b:
                for name, x, y in zip(("offsets", "hashes", "positions", "strands"), a.download(), b.download()):
                    assert x.shape == y.shape and (x == y).all(), f"k={k} w={w}: {name} differ"


def check_crafted(dev):
    sources, cases = crafted()
    want = reference_records("crafted")
    with dev.batch(sources) as sb:
        compare(dev, sb, cases, want)
        for n in (65, 129):  # more than one wavefront of lanes, more than one workgroup of wavefronts
            pick = [(7 * i) % len(cases) for i in range(n)]
            compare(dev, sb, [cases[i] for i in pick], [want[i] for i in pick])
        compare(dev, sb, [], [])
        # the sketches the comparison rests on are not empty, and a masked record's minimizers are the unmasked record's in the range
        long = next(s for s, seq in enumerate(sources) if len(seq) == 9000)
        with dev.batch_mask(sb, [long], [100], [8300]) as mb, dev.sketch(mb, 20, 10) as a, dev.batch([sources[long]]) as fb, \
                dev.sketch(fb, 20, 10) as b:
            (_, ah, ap, _), (_, bh, bp, _) = a.download(), b.download()
            assert len(ap) > 1000 and ap.min() >= 100 and ap.max() <= 8300 - 20
            inner = (bp >= 100 + 10) & (bp <= 8300 - 20 - 10)  # a window's width away from the range's ends
            assert set(zip(bh[inner].tolist(), bp[inner].tolist())) <= set(zip(ah.tolist(), ap.tolist()))
    dev.sync()


def check_random(dev):
    sources, cases = random_cases()
    with dev.batch(sources) as sb:
        compare(dev, sb, cases, reference_records("random"))
    dev.sync()


def check_refusals(dev):
    sources, cases = crafted()
    with dev.batch(sources) as sb:
        for args, text in ((([len(sources)], [0], [0]), "out of range"), (([0], [5], [4]), "above keep_hi"),
                           (([0, 1], [0, 0], [37, 1]), "beyond the source sequence")):
            with pytest.raises(capi.NtlError) as e:
                dev.batch_mask(sb, *args)
            assert e.value.code == capi.NTL_EINVAL and text in str(e.value), str(e.value)
        with pytest.raises(ValueError):
            dev.batch_mask(sb, [0, 1], [0], [1])
        long = next(s for s, seq in enumerate(sources) if len(seq) == 9000)
        mb = dev.batch_mask(sb, [long, 0], [100, 3], [8300, 30])
        sk = dev.sketch(mb, 20, 10)
        mb.close()  # destroyed right after the sketch was queued
    with dev.batch([masked(sources[long], 100, 8300), masked(sources[0], 3, 30)]) as ref, dev.sketch(ref, 20, 10) as want:
        for x, y in zip(sk.download(), want.download()):
            assert (x == y).all()
    sk.close()
    dev.sync()


# ---------------------------------------------------------------- under the SIMT mock

@pytest.fixture(scope="module")
def sim_dev():
    from sim import simlib
    dev = simlib.device()
    yield dev
    dev.close()


def test_sim_crafted(sim_dev):
    check_crafted(sim_dev)


def test_sim_random(sim_dev):
    check_random(sim_dev)


def test_sim_refusals(sim_dev):
    check_refusals(sim_dev)


# ---------------------------------------------------------------- on the GPU

@pytest.fixture(scope="module")
def gpu_dev():
    dev = capi.Device(0)
    yield dev
    dev.close()


@pytest.mark.gpu
def test_gpu_crafted(gpu_dev):
    check_crafted(gpu_dev)


@pytest.mark.gpu
def test_gpu_random(gpu_dev):
    check_random(gpu_dev)


@pytest.mark.gpu
def test_gpu_refusals(gpu_dev):
    check_refusals(gpu_dev)
