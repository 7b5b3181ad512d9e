"""Shared by tests/test_merge.py and tests/test_merge_device.py: the reference's four merge cases, a MergePlan rendered in plain
Python (slicing, bytes.translate with the stitch kernel's table, .lower()), and the crafted text of the count kernel's tests."""
import functools
import gzip
import os

import numpy as np

from ntlink_amd import capi, merge

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPECTED = os.path.join(ROOT, "tests", "golden", "ref", "expected_outputs")
CASES = {1: "scaffolds_1.fa.k32.w250.z1000", 2: "scaffolds_2.fa.k32.w100.z1000", 3: "scaffolds_3.fa.k24.w250.z1000",
         4: "scaffolds_4.fa.k40.w100.z1000"}
TABLE = bytes.maketrans(b"ACGTUNMRWSYKVHDBacgtunmrwsykvhdb", b"TGCAANKYWSRMBDHVtgcaankywsrmbdhv")
T = 16384  # COUNT_TILE of csrc/count_kernels.h (and STITCH_TILE)


def case_file(n, suffix):
    return os.path.join(EXPECTED, CASES[n] + suffix)


def trimmed_fasta(n):
    "the merge's input of case n; the reference's .trimmed_scafs.fa is kept gzip-compressed among the fixtures, the same bytes"
    return case_file(n, ".trimmed_scafs.fa.gz")


@functools.lru_cache(maxsize=None)
def golden(n):
    "the reference's merge output of case n (.stitch.abyss-scaffold.fa, kept gzip-compressed, the same bytes)"
    with gzip.open(case_file(n, ".stitch.abyss-scaffold.fa.gz"), "rb") as fh:
        return fh.read()


def read_fasta(path):
    "[(header line without `>`, sequence)] of a gzip-compressed FASTA file"
    out = []
    with gzip.open(path, "rb") as fh:
        for line in fh:
            if line[:1] == b">":
                out.append([line[1:].rstrip(b"\r\n"), []])
            else:
                out[-1][1].append(line.rstrip(b"\r\n"))
    return [(header, b"".join(parts)) for header, parts in out]


def render(plan, sequences):
    "the text of a MergePlan in plain Python; sequences: the bytes of the contigs' store, by record"
    out = []
    for header, segs, size in plan.records():
        seq = []
        for store, rec, lo, hi, flags in segs:
            if store == capi.NTL_STITCH_FILL:
                seq.append(bytes([rec]) * (hi - lo))
                continue
            assert store == 0
            piece = sequences[rec][lo:hi]
            if flags & capi.NTL_STITCH_REVCOMP:
                piece = piece[::-1].translate(TABLE)
            if flags & capi.NTL_STITCH_LOWER_FIRST:
                piece = piece[:1].lower() + piece[1:]
            seq.append(piece)
        text = header + b"".join(seq) + b"\n"
        assert len(text) == size
        out.append(text)
    return b"".join(out)


def called(text):
    "the bytes of `text` that are one of ACGTacgt, as a bool array"
    return np.isin(np.frombuffer(text, np.uint8), np.frombuffer(b"ACGTacgt", np.uint8))


def counts_of_fasta(text):
    "called bases per record of a FASTA text with one-line sequences"
    lines = text.split(b"\n")
    return np.array([int(called(seq).sum()) for seq in lines[1::2]], np.uint64)


def expected_counts(text, rec_off):
    c = np.concatenate([[0], np.cumsum(called(text))])
    off = np.asarray(rec_off, np.int64)
    return (c[off[1:]] - c[off[:-1]]).astype(np.uint64)


ALPHABET = np.frombuffer(b"ACGTACGTACGTacgtNnUu\n>RYKMSWBDHVryXx*-@[`{\x00\xc1\xe7", np.uint8)


@functools.lru_cache(maxsize=None)
def count_cases():
    """(text, {name: rec_off}): one crafted text of a few tiles, whose length is no multiple of 16, and the ways it is cut into records"""
    rng = np.random.default_rng(5)
    text = ALPHABET[rng.integers(0, len(ALPHABET), 5 * T + 1003)].tobytes()
    n = len(text)
    assert n % 16 != 0
    cases = {}
    # lengths 0, 1, 15, 16, 17 (and a few more) in a row, from offset 0 and from an odd offset
    lens = [0, 1, 15, 16, 17, 0, 0, 31, 32, 33, 1, 1, 0, 255, 256, 257]
    cases["small_lengths"] = np.concatenate([[0], np.cumsum(lens)])
    cases["small_lengths_odd_start"] = 7 + cases["small_lengths"]
    # a record ending exactly on a tile boundary, the next one starting there; one record over three tiles
    cases["tile_boundary"] = [0, 100, T, T + 5, 2 * T, n]
    cases["three_tiles"] = [T - 3, 3 * T + 9]
    cases["three_tiles_aligned"] = [T, 4 * T]
    # more than 64 one-byte records in one tile (and in one lane's chunks): 200 of them, then the rest
    cases["one_byte_records"] = list(range(T + 40, T + 241)) + [n]
    # every byte of a tile a record of its own, with empty records between them
    cases["every_byte"] = np.repeat(np.arange(2 * T - 100, 2 * T + 300), 2)
    # the whole text as one record; as two; a start behind the first tile; an end before the last byte; empty records at both ends
    cases["whole"] = [0, n]
    cases["halves"] = [0, n // 2 + 1, n]
    cases["inner"] = [2 * T + 17, 2 * T + 17, 4 * T - 1, n - 3, n - 3]
    cases["last_chunk"] = [n - 11, n - 4, n]
    cases["all_empty"] = [500, 500, 500]
    cases["random"] = np.sort(rng.integers(0, n + 1, 400))
    # a FASTA-like cut: header, sequence, newline + header, sequence, ...
    cases["fasta_like"] = [0, 12, 12 + T + 100, 12 + T + 113, 4 * T, 4 * T + 14, n - 1, n]
    return text, {name: np.asarray(off, np.uint64) for name, off in cases.items()}


@functools.lru_cache(maxsize=None)
def count_reference():
    "the expected counts of every case: computed once, shared"
    text, cases = count_cases()
    return {name: expected_counts(text, off) for name, off in cases.items()}
