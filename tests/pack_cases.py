"""Crafted and random batches for the device-side ingest (tests/test_pack_device.py): ASCII -> 2-bit bases + the table of ACGT runs, made by
the six kernels of csrc/pack_kernels.h under ntl_batch_create, and what the packed constructors build from the host parser's tables.

The reference is plain Python over the input bytes -- no device, no library:
  text        c & 0xDF for the eight bytes ACGTacgt, N for every other byte value; offsets are the cumulative lengths
  runs        the maximal runs of those eight bytes inside each sequence (never across a sequence boundary)
  k-mer starts every i whose k bytes from i lie in one run: what a sketch at w = 1 holds, one minimizer per valid k-mer
  pure        every sequence is non-empty and one run of its whole length: what Batch.download() and synth_slices demand

A batch shows its run table through the existing calls only: download_n() shows which bases a run covers and their codes; the sketches
at (k, w) = (3, 1) and (4, 2) tell one run from two adjacent ones (a k-mer across the seam exists or does not) and a right any_multi from
a wrong one (the kernels are launched without their multi-run path); download() shows the purity flag."""
import functools

import numpy as np
import pytest

import oracle
from ntlink_amd import capi

# the geometry of pack_kernels.h, ntl_hip.hip and scan_kernels.h that the crafted lengths are about
LEAD_PAD = 16                  # NTL_LEAD_PAD: zero positions in front of the first base, so global position = 16 + base index
WORD = 16                      # bases per packed u32: pack16 handles one word, by a 16-byte load or by its byte loop
GROUP = 32                     # positions per thread: one word of valid32 / ss32 / starts32
PACK_NT = 256                  # threads per block
BLOCK = PACK_NT * GROUP        # 8192 positions per block
SCAN_TILE = 256 * 8            # SCAN_NT * SCAN_IPT: per-thread start counts (one per group) that one tile of scan_launch scans

VALID = frozenset(b"ACGTacgt")
ACGT = np.frombuffer(b"ACGT", np.uint8)
KW = ((3, 1), (4, 2))
SWEEP = 70                     # places 0..69 of the bit sweep: two groups and a bit more
MAX_RANDOM = 200


# ---------------------------------------------------------------- the plain reference

def text_of(seqs):
    """-> (bytes of download_n(), offsets)"""
    text = b"".join(bytes(c & 0xDF if c in VALID else 78 for c in s) for s in seqs)
    return text, np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)


def runs_of(seq):
    """[(start, length)] of the maximal runs of valid bytes"""
    runs, start = [], None
    for i, c in enumerate(seq):
        if c in VALID:
            if start is None:
                start = i
        elif start is not None:
            runs.append((start, i - start))
            start = None
    if start is not None:
        runs.append((start, len(seq) - start))
    return runs


def kmer_starts(seq, k):
    return [i for start, n in runs_of(seq) for i in range(start, start + n - k + 1)]


def is_pure(seqs):
    return all(len(s) > 0 and runs_of(s) == [(0, len(s))] for s in seqs)


@functools.lru_cache(maxsize=None)
def reference(seqs, k):
    """(text, offsets, k-mer starts per sequence, pure) of a tuple of byte strings: computed once, shared by every test and form"""
    return text_of(seqs) + ([kmer_starts(s, k) for s in seqs], is_pure(seqs))


def rand(rng, n):
    return ACGT[rng.integers(0, 4, n)].tobytes()


def draw(rng, alphabet, n):
    return np.frombuffer(alphabet, np.uint8)[rng.integers(0, len(alphabet), n)].tobytes()


# ---------------------------------------------------------------- crafted batches: name -> list of byte strings

def sweep_sequences():
    """Short sequences (70 to 100 bases) that put one run start, one run end or both at every place 0..69 of a sequence, and sequence
    boundaries between two valid bases."""
    rng = np.random.default_rng(1)
    seqs = []
    for p in range(SWEEP):
        n = SWEEP + 1 + p % 30                      # 71..100: the boundaries behind these walk through the groups as well
        hole = bytearray(rand(rng, n)); hole[p] = 78
        one = bytearray(b"N" * n); one[p] = ACGT[p % 4]
        two = bytearray(b"N" * n); two[p:p + 2] = rand(rng, 2)
        both = bytearray(rand(rng, n)); both[p] = 78; both[p + 1 + p % 3] = 78     # a run of 0, 1 or 2 bases between two N
        seqs += [bytes(hole), bytes(one), bytes(two), bytes(both)]
        if p % 7 == 0:
            # ... valid | valid ...: the run ends at the sequence-start bit while the valid bits run on
            seqs += [rand(rng, n), rand(rng, SWEEP + p % 5), b"N" * (n - 1) + b"G", b"T" + b"N" * (n - 1), rand(rng, n - 1) + b"N", rand(rng, n)]
    assert all(SWEEP <= len(s) <= 100 for s in seqs)
    return seqs


@functools.lru_cache(maxsize=None)
def bit_sweep():
    """32 batches: the sweep behind a first sequence of r random bases, r = 0..31 -- every start, end and boundary meets every bit of a
    32-position group, both of its packed words, and bit 31 -> bit 0 across two threads"""
    body = sweep_sequences()
    rng = np.random.default_rng(2)
    return [(f"sweep r={r}", [rand(rng, r)] + body) for r in range(GROUP)]


@functools.lru_cache(maxsize=None)
def degenerate():
    rng = np.random.default_rng(3)
    a, b, c = rand(rng, 21), rand(rng, 40), rand(rng, 13)
    return [("no sequences", []), ("one empty", [b""]), ("only empty", [b"", b"", b""]),
            ("empty first, doubled inside, last", [b"", a, b"", b"", b, b""]),      # sets the same bit of ss32 two and three times
            ("empty twice at the front and the end", [b"", b"", a, b, b"", b""]),
            ("all-N between two valid", [a, b"N" * 33, b]), ("all-N alone", [b"N" * 50]), ("all-N, a group long", [c, b"N" * GROUP, a]),
            ("A", [b"A"]), ("N", [b"N"]), ("A N A", [b"A", b"N", b"A"]), ("ANA N", [b"ANA", b"N"]),
            ("leading N", [b"NACG", b"ACGT"]), ("trailing N", [b"ACGN", b"ACGT"]), ("lower case", [b"acgt"]),
            ("pure", [a, b, c]), ("pure, one sequence", [rand(rng, 100)]), ("pure with an empty one", [a, b"", b])]


@functools.lru_cache(maxsize=None)
def tails():
    """LEAD_PAD + total = 0, 1, 15, 16, 17, 31 modulo 32: the last word packed by the 16-byte load or by the byte loop, seq_base[nseq] in
    the last group or in the zero word behind it; the last sequence ends valid, or in N"""
    rng = np.random.default_rng(4)
    out = []
    for m in (0, 1, WORD - 1, WORD, WORD + 1, GROUP - 1):
        total = 3 * GROUP - LEAD_PAD + m
        assert (LEAD_PAD + total) % GROUP == m
        s = rand(rng, total)
        out += [(f"tail {m} valid", [s[:37], s[37:]]), (f"tail {m} N", [s[:37], s[37:-1] + b"N"]), (f"tail {m} one sequence", [s]),
                (f"tail {m} valid, N before", [s[:37], s[37:-2] + b"N" + s[-1:]])]
    return out


@functools.lru_cache(maxsize=None)
def seams():
    """Totals that end one base before, at and one behind the first block's last position, and at the second block's; a sequence boundary
    one before, at and one behind the block seam, with and without empty sequences on it; pure bases (the boundary alone ends the run) and
    short runs.  Then one batch of SCAN_TILE + 1 groups with short runs all along: starts in both tiles of the scan."""
    rng = np.random.default_rng(5)
    out = []
    seam = BLOCK - LEAD_PAD  # the base at global position 8192: the first of block 1
    for total in (seam - 1, seam, seam + 1, 2 * BLOCK - LEAD_PAD):
        for kind, s in (("pure", rand(rng, total)), ("runs", draw(rng, b"ACGTACGTN", total))):
            for d in (-1, 0, 1):
                cut = min(seam + d, total)
                out.append((f"seam total={total} {kind} boundary at {cut}", [s[:cut], s[cut:]]))
                if kind == "runs" or d == 0:
                    out.append((f"seam total={total} {kind} empty ones at {cut}", [s[:cut], b"", b"", s[cut:]]))
    total = (SCAN_TILE + 1) * GROUP - LEAD_PAD
    s = draw(rng, b"ACGTACGTACGTN", total)
    assert len(runs_of(s[:total // 2])) > 100 and len(runs_of(s[total - 40:])) >= 1
    out.append((f"scan: {SCAN_TILE} + 1 groups", [s[:40000], s[40000:]]))
    return out


@functools.lru_cache(maxsize=None)
def every_byte():
    return [("bytes 0..255 and back", [bytes(range(256)), bytes(range(255, -1, -1))])]


ALPHABETS = (b"ACGT", b"ACGTN", b"ACGTacgtNnRYKM", b"AN", bytes(range(256)))
LENGTHS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 63, 64, 65)


@functools.lru_cache(maxsize=None)
def random_batches(n=100):
    """20 batches per alphabet, half of them with lengths around the word and group sizes (a batch costs a third of a second under the
    mock, most of it the two sketches)"""
    assert n <= MAX_RANDOM and n % (2 * len(ALPHABETS)) == 0
    out = []
    for seed in range(n):
        rng = np.random.default_rng(1000 + seed)
        alphabet = ALPHABETS[seed % len(ALPHABETS)]
        nseq = int(rng.integers(0, 12))
        if (seed // len(ALPHABETS)) % 2:
            lens = rng.integers(0, 100, nseq).tolist()
        else:
            lens = [LENGTHS[i] for i in rng.integers(0, len(LENGTHS), nseq)]
        out.append((f"random seed={seed}", [draw(rng, alphabet, n) for n in lens]))
    return out


def letter_cases():
    """what a FASTA file can hold (no arbitrary bytes, '>' or newlines): one shift of the sweep, the degenerate cases and the tails"""
    return [bit_sweep()[5]] + degenerate() + tails()


# ---------------------------------------------------------------- the checks

@functools.lru_cache(maxsize=None)
def _oracle_sketch(seqs, k, w):
    text = b"".join(seqs)
    return oracle.sketch_batch(text, np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64), k, w)


def check_layout(dev, b, seqs, name):
    """batch b holds seqs: sizes, every base, the run table as the sketches show it"""
    seqs = tuple(seqs)
    text, off, starts, _pure = reference(seqs, KW[0][0])
    assert (b.nseq, b.bases) == (len(seqs), len(text)), name
    buf, got_off = b.download_n()
    assert got_off.tolist() == off.tolist(), name
    got = buf.tobytes()
    if got != text:
        at = next(i for i in range(len(text)) if got[i] != text[i])
        raise AssertionError(f"{name}: download_n differs first at base {at} (global position {LEAD_PAD + at}): "
                             f"{got[max(at - 8, 0):at + 8]!r}, expected {text[max(at - 8, 0):at + 8]!r}")
    for k, w in KW:
        with dev.sketch(b, k, w) as sk:
            moff, mh, mp, ms = sk.download()
        if (k, w) == KW[0]:
            assert np.diff(moff.astype(np.int64)).tolist() == [len(x) for x in starts], f"{name}: k-mers per sequence at k={k}"
            assert mp.tolist() == [i for x in starts for i in x], f"{name}: k-mer positions at k={k}"
        for what, x, y in zip(("offsets", "hashes", "positions", "strands"), (moff, mh, mp, ms), _oracle_sketch(seqs, k, w)):
            assert x.shape == y.shape and (x == y).all(), f"{name}: k={k} w={w}: {what} differ from the oracle's"


def check_download(b, seqs, name):
    """download(): the bytes and offsets that went in (upper-cased) for a pure batch, refusal for every other"""
    text, off, _starts, pure = reference(tuple(seqs), KW[0][0])
    if pure:
        buf, got_off = b.download()
        assert buf.tobytes() == text == b"".join(seqs).upper() and got_off.tolist() == off.tolist(), name
    else:
        with pytest.raises(capi.NtlError) as e:
            b.download()
        assert e.value.code == capi.NTL_EINVAL and "pure-ACGT" in str(e.value), f"{name}: {e.value}"


def check_cases(dev, cases):
    for name, seqs in cases:
        with dev.batch(seqs) as b:
            check_layout(dev, b, seqs, name)
            check_download(b, seqs, name)
    dev.sync()


def check_first_offset(dev):
    """offsets[0] = 5 and = 16: the bases in front of it are not the batch's (valid ones here, so that a batch that began at byte 0, or
    packed from there, would show them)"""
    rng = np.random.default_rng(6)
    some = ("only empty", "empty first, doubled inside, last", "all-N between two valid", "N", "leading N", "pure")
    cases = [c for c in degenerate() if c[0] in some] + tails()[::4]  # every residue of the total, the last sequence ending valid
    assert len(cases) == len(some) + 6
    for o0 in (5, WORD):
        for name, seqs in cases:
            buf = np.frombuffer(rand(rng, o0) + b"".join(seqs), np.uint8)
            off = text_of(seqs)[1] + np.uint64(o0)
            with dev.batch(buf, off) as b:
                check_layout(dev, b, seqs, f"offsets[0]={o0}: {name}")
                check_download(b, seqs, f"offsets[0]={o0}: {name}")
    dev.sync()


def packed_batches(dev, path, nseq):
    """the records of a FASTA file through ntl_batch_create_packed (the two-pass packing reader) and ntl_batch_create_packed_at (the
    one-pass reader).  The readers yield nothing for a file without records: such a set is written out as they lay one out."""
    from ntlink_amd import seqio
    if nseq:
        two_pass = seqio.load_all([path], packed=True)
        one_pass, = seqio.load([path], max_bases=1 << 20, packed=True)
    else:
        none = dict(packed=np.zeros(int(capi.load().ntl_packed_words(0)), np.uint32),
                    runs=(np.zeros(1, np.uint32), np.zeros(0, np.uint32), np.zeros(0, np.uint32)))
        two_pass = seqio.SeqSet([], None, np.zeros(1, np.uint64), **none)
        one_pass = seqio.SeqSet([], None, np.zeros(1, np.uint64), positions=np.zeros(0, np.uint64), span_positions=0, **none)
    assert len(two_pass) == len(one_pass) == nseq and two_pass.positions is None and one_pass.positions is not None
    return (("packed", dev.batch_packed(two_pass)), ("packed-at", dev.batch_packed(one_pass)))


def check_packed_constructors(dev, tmp_path):
    for i, (name, seqs) in enumerate(letter_cases()):
        path = tmp_path / f"case{i}.fa"
        with open(path, "wb") as fh:
            for j, s in enumerate(seqs):
                fh.write(b">s%d\n" % j + s + b"\n")
        for form, b in packed_batches(dev, str(path), len(seqs)):
            with b:
                check_layout(dev, b, seqs, f"{form}: {name}")
                check_download(b, seqs, f"{form}: {name}")
    dev.sync()


def check_guards(dev):
    """the four batches whose run count does not give them away, by name; the other users of the purity flag: synth_slices refuses an
    impure source, a masked batch is pure only where every record keeps its one whole run, a synthetic batch always is"""
    rng = np.random.default_rng(7)
    for seqs in ([b"NACG", b"ACGT"], [b"ACGN", b"ACGT"], [b"ANA", b"N"]):
        with dev.batch(seqs) as b:
            assert b.download_n()[0].tobytes() == b"".join(seqs)
            with pytest.raises(capi.NtlError) as e:
                b.download()
            assert "pure-ACGT" in str(e.value)
    with dev.batch([b"acgt"]) as b:
        buf, off = b.download()
        assert buf.tobytes() == b"ACGT" and off.tolist() == [0, 4]
    first, second = rand(rng, 60), rand(rng, 64)
    for src in ([b"NACG" + first, second], [first + b"ACGN", second], [second, b"ACG" + first + b"N"]):
        with dev.batch(src) as sb:
            with pytest.raises(capi.NtlError) as e:
                dev.synth_slices(sb, 1, [1], [0], [32])
            assert e.value.code == capi.NTL_EINVAL and "must be pure ACGT" in str(e.value)
    with dev.batch([first, second]) as sb:
        with dev.synth_slices(sb, 1, [1, 0], [3, 0], [32, 60]) as sl:   # ... and takes a pure one, bases as they are
            assert sl.download()[0].tobytes() == second[3:35] + first
        for lo, hi, pure in (([0, 0], [60, 64], True), ([0, 1], [60, 64], False), ([0, 0], [59, 64], False), ([0, 0], [60, 0], False)):
            with dev.batch_mask(sb, [0, 1], lo, hi) as mb:
                want = [b"N" * a + s[a:z] + b"N" * (len(s) - z) for s, a, z in zip((first, second), lo, hi)]
                assert mb.download_n()[0].tobytes() == b"".join(want)
                check_download(mb, want, f"masked {lo} {hi}")
                assert is_pure(want) == pure
    with dev.batch([first + b"N" + second]) as sb, dev.batch_mask(sb, [0, 0], [0, 61], [60, 125]) as mb:
        check_download(mb, [first + b"N" * 65, b"N" * 61 + second], "masked: one run each, neither whole")  # as many runs as records
    with dev.synth_genome(9, [1, 33, 100]) as g:
        buf, off = g.download()
        assert off.tolist() == [0, 1, 34, 134] and set(buf.tobytes()) <= set(b"ACGT")
        assert g.download_n()[0].tobytes() == buf.tobytes()
    dev.sync()
