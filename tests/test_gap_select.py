"""Which read fills which gap, decided on the device: gapfill.choose_gap_reads over the native verbose-mapping reader (formats.read_verbose ->
ntl_vmap_*, csrc/ntl_io.cpp) and Device.gap_select (ntl_gap_select, csrc/gap_select_kernels.h) -- under the SIMT mock and on the GPU, the
same checks.
  a. golden: choose_gap_reads against what the reference's own read_path_file_pairs, read_verbose_mappings, choose_best_read_per_pair and
     find_masking_cut_points leave in every pair (tests/golden/gen/gapsel_cases.json.gz, made by tests/golden/gen_goldens_gapsel.py), the
     file whole and in blocks of a few reads
  b. random reads: the device's candidate records, record for record, against gapfill.restated_candidates on the same file; and the end
     state of choose_gap_reads against choose_gap_reads_restated (the reference's assertion included)
  c. the reader's arrays against formats.parse_verbose on those files, and its four refusals with their line numbers
  d. the refusals of the device call: a pair table more than half full, a read with a contig twice
  e. a pair table with chosen keys: 20 pairs of one home across the end of a table of 64 slots, 6 of another, exactly half full; reads of
     present pairs, of their reverse complements, of absent pairs whose probes walk the cluster to the empty slot behind it, and one of
     five mappings -- against restated_candidates record for record, the table itself against a linear-probe simulation"""
import argparse
import functools
import gzip
import itertools
import json
import os
import re
import types

import numpy as np
import pytest

from helpers import assert_reader_blocks, parsed_verbose_arrays
from ntlink_amd import capi, formats, gapfill

HERE = os.path.dirname(os.path.abspath(__file__))
SMALL_BLOCK = 600  # bytes of text per block: a few reads, so that the files are cut in many places


def _write(tmp_path, name, text):
    path = str(tmp_path / name)
    with open(path, "w") as fh:
        fh.write(text)
    return path


def _state(pairs):
    return {f"{s} {t}": [sorted(p.mapping_reads), p.chosen_read, p.source_ctg_cut, p.source_read_cut, p.target_ctg_cut, p.target_read_cut]
            for (s, t), p in pairs.items()}


def _sequences(lengths):
    return {name: types.SimpleNamespace(length=length) for name, length in lengths.items()}


# ---------------------------------------------------------------- a. golden

@functools.lru_cache(maxsize=None)
def golden():
    with gzip.open(os.path.join(HERE, "golden", "gen", "gapsel_cases.json.gz"), "rt") as fh:
        return json.load(fh)


def check_golden(dev, tmp_path, max_bytes):
    doc = golden()
    vp, pp = _write(tmp_path, "g.verbose_mapping.tsv", doc["verbose"]), _write(tmp_path, "g.path", doc["path"])
    pairs = gapfill.read_path_file_pairs(pp, doc["min_gap"])
    assert [f"{s} {t}" for s, t in pairs] == list(doc["pairs"]), "read_path_file_pairs: the reference's pairs, in its order"
    assert doc["tags"]["small_gap"] not in doc["pairs"]
    if max_bytes:
        assert sum(1 for _ in formats.read_verbose(vp, ["x"], max_bytes=max_bytes, lib_path=dev.lib_path)) > 20
    gapfill.choose_gap_reads(pairs, vp, _sequences(doc["lengths"]), argparse.Namespace(large_k=doc["large_k"]), dev=dev,
                             max_bytes=max_bytes or gapfill.VERBOSE_BLOCK_BYTES)
    got = _state(pairs)
    for key, want in doc["pairs"].items():
        assert got[key] == want, f"pair {key}: {got[key]}, the reference leaves {want}"
    # the fixture's own reach
    want = doc["pairs"]
    assert want[doc["tags"]["by_name"]][:2] == [["read10", "read9"], "read9"], "decided by the name, as a string"
    assert want[doc["tags"]["second"]][:2] == [["u_best", "u_second"], "u_second"], "the first candidate invalid"
    assert want[doc["tags"]["revcomp"]][1] == "rc_read", "supported through the reverse complement"
    assert want[doc["tags"]["none_valid"]][:2] == [["v_far"], None], "supported, and no read chosen"
    dev.sync()


# ---------------------------------------------------------------- b. random reads

N_CTG, N_PAIRS, N_READS, K = 40, 30, 300, 40
HIT_COUNTS = (1, 2, 63, 64, 65, 150)


def _hits(rng, n, ctg_len, rpos, plus, spoil):
    """n hits of one mapping: one orientation and monotone contig positions -- near either end of the contig (past it at times, where
    the reference's assertion fails) -- unless `spoil` asks for mixed strands (1) or a position out of order (2)"""
    step = int(rng.integers(3, 40))
    where = rng.random()
    if where < 0.4:
        c0 = int(rng.integers(0, 60))
    elif where < 0.8:
        c0 = max(0, ctg_len - K - n * step - int(rng.integers(-80, 60)))
    else:
        c0 = int(rng.integers(0, ctg_len))
    cpos = c0 + step * np.arange(n)
    if rng.random() < 0.5:
        cpos = cpos[::-1]
    rs = rng.integers(0, 2, n)
    cs = rs if plus else 1 - rs
    cpos, cs = cpos.copy(), cs.copy()
    if spoil == 1:    # one hit on the other strand
        cs[int(rng.integers(0, n))] ^= 1
    elif spoil == 2:  # one position repeated: neither increasing nor decreasing
        i = int(rng.integers(1, n))
        cpos[i] = cpos[i - 1]
    rp = rpos + 25 * np.arange(n)
    return " ".join(f"{c}:{'+' if a else '-'}_{r}:{'+' if b else '-'}" for c, a, r, b in zip(cpos.tolist(), cs.tolist(), rp.tolist(), rs.tolist())), int(rp[-1])


@functools.lru_cache(maxsize=None)
def random_case(seed=7):
    """(verbose text, path text, lengths): about 300 reads of up to 6 mappings over 40 contigs in the path's 30 pairs and 8 contigs that
    are in no pair (unknown names to the reader's table).  Two reads in three meet a pair's two contigs, directly or as its reverse
    complement, with other mappings between and around them; a third of all mappings of two hits and more is made invalid, by its
    strands or by its positions.  Hit counts: 1, 2, 63, 64, 65, 150."""
    rng = np.random.default_rng(seed)
    lengths = {f"ctg{i}": int(rng.integers(6000, 60000)) for i in range(N_CTG)}
    lengths.update({f"other{i}": int(rng.integers(6000, 60000)) for i in range(8)})
    names = list(lengths)
    pair_list, path = [], []
    while len(pair_list) < N_PAIRS:
        a, b = rng.choice(N_CTG, 2, replace=False).tolist()
        pair = (f"ctg{a}" + "+-"[int(rng.integers(0, 2))], f"ctg{b}" + "+-"[int(rng.integers(0, 2))])
        if pair not in pair_list:
            pair_list.append(pair)
            path.append(f"path{len(path)}\t{pair[0]} {int(rng.integers(100, 5000))}N {pair[1]}")
    flip = {"+": "-", "-": "+"}
    rows = []
    for r in range(N_READS):
        nodes = []
        if rng.random() < 0.67:
            s, t = pair_list[int(rng.integers(0, N_PAIRS))]
            nodes = [s, t] if rng.random() < 0.5 else [t[:-1] + flip[t[-1]], s[:-1] + flip[s[-1]]]
        for _ in range(int(rng.integers(0 if nodes else 1, 5))):
            name = names[int(rng.integers(0, len(names)))]
            if all(name != n[:-1] for n in nodes):
                nodes.insert(int(rng.integers(0, len(nodes) + 1)), name + "+-"[int(rng.integers(0, 2))])
        rpos = int(rng.integers(0, 3000))
        for node in nodes:
            n = HIT_COUNTS[int(rng.integers(0, len(HIT_COUNTS)))] + (int(rng.integers(0, 60)) if rng.random() < 0.1 else 0)
            spoil = int(rng.integers(1, 3)) if n > 1 and rng.random() < 0.4 else 0
            toks, last = _hits(rng, n, lengths[node[:-1]], rpos, node[-1] == "+", spoil)
            rows.append(f"read{r}\t{node[:-1]}\t{int(rng.integers(1, 200))}\t{toks}")
            rpos = last + int(rng.integers(50, 4000))
    return "".join(row + "\n" for row in rows), "".join(row + "\n" for row in path), lengths


def test_random_case_reach(tmp_path):
    """the restatement alone, on the CPU: the random file gives what the comparison below relies on"""
    verbose, path, lengths = random_case()
    vp, pp = _write(tmp_path, "r.verbose_mapping.tsv", verbose), _write(tmp_path, "r.path", path)
    pairs = gapfill.read_path_file_pairs(pp, 20)
    assert len(pairs) == N_PAIRS
    want, ids = gapfill.restated_candidates(pairs, vp, _sequences(lengths), K)
    assert len(ids) == N_READS and len(set(want["read"].tolist())) >= N_READS // 5, "at least 20 % of the reads give a candidate"
    assert set(want["flags"].tolist()) == set(range(8)), sorted(set(want["flags"].tolist()))
    with open(vp) as fh:
        parsed = list(formats.parse_verbose(fh))
    n_hits = {len(h) for _rid, entries in parsed for _ctg, h in entries}
    assert {1, 2, 63, 64, 65} <= n_hits and max(n_hits) > 128
    assert max(len(entries) for _rid, entries in parsed) == 6
    n_maps = sum(len(entries) for _rid, entries in parsed)
    n_valid = sum(len(order) for _rid, _info, order in gapfill._restated_mappings(vp))
    assert 0.2 < 1 - n_valid / n_maps < 0.45, "about a third of the mappings is invalid"
    assert any(ctg.startswith("other") for _rid, entries in parsed for ctg, _h in entries)


def check_random(dev, tmp_path):
    verbose, path, lengths = random_case()
    vp, pp = _write(tmp_path, "r.verbose_mapping.tsv", verbose), _write(tmp_path, "r.path", path)
    sequences = _sequences(lengths)
    pairs = gapfill.read_path_file_pairs(pp, 20)
    want, ids = gapfill.restated_candidates(pairs, vp, sequences, K)
    ctg_names, ctg_len, keys = gapfill.pair_tables(pairs, sequences)
    for max_bytes in (0, 5000):
        got, first, names = [], 0, []
        for block, cands in gapfill.gap_candidates(vp, ctg_names, ctg_len, keys, K, dev=dev, max_bytes=max_bytes):
            cands["read"] += first
            first += len(block.names)
            names += block.names.tolist()
            got.append(cands)
        got = np.concatenate(got)
        assert names == ids and len(got) == len(want), (len(got), len(want))
        for i in np.flatnonzero(got != want)[:5]:
            raise AssertionError(f"max_bytes {max_bytes}, record {i}: {got[i]}, the restated reference gives {want[i]}")
    # the end state: the reference's assertion where it reaches a negative distance, the same pairs either way
    args = argparse.Namespace(large_k=K)
    mine, theirs = gapfill.read_path_file_pairs(pp, 20), gapfill.read_path_file_pairs(pp, 20)
    with pytest.raises(AssertionError):
        gapfill.choose_gap_reads_restated(theirs, vp, sequences, args)
    with pytest.raises(AssertionError):
        gapfill.choose_gap_reads(mine, vp, sequences, args, dev=dev)
    # without the reads whose distance comes out negative both run through
    bad = {ids[r] for r in want["read"][(want["flags"] & capi.NTL_GAPSEL_NEGATIVE) != 0].tolist()}
    vq = _write(tmp_path, "q.verbose_mapping.tsv", "".join(row + "\n" for row in verbose.splitlines() if row.split("\t")[0] not in bad))
    mine, theirs = gapfill.read_path_file_pairs(pp, 20), gapfill.read_path_file_pairs(pp, 20)
    gapfill.choose_gap_reads_restated(theirs, vq, sequences, args)
    gapfill.choose_gap_reads(mine, vq, sequences, args, dev=dev, max_bytes=5000)
    assert _state(mine) == _state(theirs)
    chosen = [p for p in theirs.values() if p.chosen_read is not None]
    # what this end state decides: a third of the pairs at least get a read, some of them one among several, and some supported pair none
    assert len(chosen) >= N_PAIRS // 3 and any(len(p.mapping_reads) > 1 for p in chosen)
    assert any(p.chosen_read is None and p.mapping_reads for p in theirs.values())
    dev.sync()


# ---------------------------------------------------------------- c. the reader

def check_reader(lib_path, tmp_path, monkeypatch):
    doc = golden()
    files = [(_write(tmp_path, "g.tsv", doc["verbose"]), sorted(doc["lengths"])[::2]),
             (_write(tmp_path, "r.tsv", random_case()[0]), [f"ctg{i}" for i in range(N_CTG)]),
             (_write(tmp_path, "n.tsv", doc["verbose"].rstrip("\n")), [])]  # no newline at the end, no contig known
    for threads_env in (None, "64"):  # one range per block; ranges of a few lines on the worker pool
        if threads_env:
            monkeypatch.setenv("NTL_IO_MIN_CHUNK", threads_env)
        for path, ctg_names in files:
            want = parsed_verbose_arrays(path, ctg_names)
            for max_bytes in (0, SMALL_BLOCK):
                blocks = list(formats.read_verbose(path, ctg_names, max_bytes=max_bytes, lib_path=lib_path))
                assert len(blocks) == 1 if not max_bytes else len(blocks) > 20
                assert_reader_blocks(blocks, want)
    assert (want[2]["ctg"] == capi.NO_CTG).all()
    # the same id again further on is another read; consecutive lines of one id stay together whatever the block size
    path = _write(tmp_path, "again.tsv", "a\tc\t1\t1:+_2:+\nb\tc\t1\t1:+_2:+\na\tc\t1\t1:+_2:+\n" + "long\tc\t1\t1:+_2:+\n" * 200)
    blocks = list(formats.read_verbose(path, ["c"], max_bytes=100, lib_path=lib_path))
    assert [n for b in blocks for n in b.names.tolist()] == ["a", "b", "a", "long"] and int(blocks[-1].map_off[-1]) == 200


GOOD = "r1\tc1\t2\t10:+_20:+ 30:+_40:+\n"
REFUSED = [  # (the bad line, what the message names)
    ("r2\tc1\t2\n", "four tab-separated fields"),
    ("r2\tc1\t2\t10:+_20:+\textra\n", "four tab-separated fields"),
    ("\n", "four tab-separated fields"),
    ("r2\tc1\t2\t10:+_20:+  30:+_40:+\n", "token"),   # an empty token
    ("r2\tc1\t2\t10:+_20\n", "token"),
    ("r2\tc1\t2\t10:x_20:+\n", "token"),
    ("r2\tc1\t2\t10:+20:+\n", "token"),
    ("r2\tc1\t2\t10:+_4294967296:+\n", "token"),      # a number above 2^32 - 1
    ("r2\tc1\t2\t99999999999:+_1:+\n", "token"),
    ("r2\tc1\t4294967296\t10:+_20:+\n", "column 3"),
    ("r2\tc1\ttwo\t10:+_20:+\n", "column 3"),
]


def check_reader_refusals(lib_path, tmp_path):
    for n_good in (0, 3, 40):  # the bad line first, in the first block, and blocks later
        for bad, what in REFUSED:
            path = _write(tmp_path, "bad.tsv", "".join(GOOD.replace("r1", f"r{i}") for i in range(n_good)) + bad + GOOD)
            for max_bytes in (0, 100):
                with pytest.raises(ValueError, match=rf"line {n_good + 1}: .*{what}"):
                    list(formats.read_verbose(path, ["c1"], max_bytes=max_bytes, lib_path=lib_path))
    path = _write(tmp_path, "edge.tsv", "r\tc1\t4294967295\t4294967295:-_4294967295:+")  # the largest numbers, no newline
    (b,) = formats.read_verbose(path, ["c0", "c1"], lib_path=lib_path)
    assert b.anchors.tolist() == [0xFFFFFFFF] and b.hits.tolist()[0][:4] == (0xFFFFFFFF, 0xFFFFFFFF, 0, 1) and b.maps["ctg"].tolist() == [1]


# ---------------------------------------------------------------- d. refusals of the device call

def check_refusals(dev, tmp_path):
    def refused(block, ctg_len, table, code=capi.NTL_EINVAL):
        with pytest.raises(capi.NtlError) as e:
            dev.gap_select(block, ctg_len, K, table)
        assert e.value.code == code and len(str(e.value)) > len("error -1: "), str(e.value)

    text = "r0\tc0\t3\t10:+_20:+ 30:+_40:+\nr0\tc1\t3\t10:+_90:+\nr0\tc2\t3\t10:-_190:+\n"
    (block,) = formats.read_verbose(_write(tmp_path, "ok.tsv", text), ["c0", "c1", "c2"], lib_path=dev.lib_path)
    ctg_len = np.array([1000, 1000, 1000], np.uint32)
    keys = [capi.pair_key(0, 0, 1, 0), capi.pair_key(1, 0, 2, 1)]
    table = capi.pair_table(keys, lib_path=dev.lib_path)
    assert len(table[0]) == 4 and dev.gap_select(block, ctg_len, K, table)["pair"].tolist() == [0, 1]
    three = capi.pair_table(keys + [capi.pair_key(0, 0, 2, 1)], lib_path=dev.lib_path)  # two lanes of one step hold a candidate
    assert dev.gap_select(block, ctg_len, K, three)["pair"].tolist() == [0, 2, 1]
    with pytest.raises(ValueError):
        capi.pair_table(keys + [capi.pair_key(2, 0, 0, 0)], n_slots=4, lib_path=dev.lib_path)
    full = (table[0].copy(), table[1].copy())
    free = int(np.flatnonzero(full[0] == np.uint64(0xFFFFFFFFFFFFFFFF))[0])
    full[0][free], full[1][free] = capi.pair_key(2, 0, 0, 0), 2
    refused(block, ctg_len, full)  # three pairs in four slots
    refused(block, ctg_len, (np.resize(table[0], 6), np.resize(table[1], 6)))  # no power of two
    assert len(dev.gap_select(block, ctg_len, K, capi.pair_table(keys, n_slots=64, lib_path=dev.lib_path))) == 2
    # a read with a contig twice (both mappings valid): a dict overwrite in the reference
    twice = text + "r0\tc0\t3\t500:+_600:+\n"
    (block2,) = formats.read_verbose(_write(tmp_path, "twice.tsv", twice), ["c0", "c1", "c2"], lib_path=dev.lib_path)
    refused(block2, ctg_len, table)
    # ... but an invalid second mapping of a contig is skipped, as in the reference
    (block3,) = formats.read_verbose(_write(tmp_path, "skipped.tsv", text + "r0\tc0\t3\t500:+_600:+ 700:-_800:+\n"), ["c0", "c1", "c2"],
                                     lib_path=dev.lib_path)
    assert dev.gap_select(block3, ctg_len, K, table)["pair"].tolist() == [0, 1]
    # offsets that do not fit the mappings
    block.map_off = np.array([0, 2], np.uint32)
    refused(block, ctg_len, table)
    # the drop-in: a contig of the path that is not in `sequences`; the same read id in two groups of lines
    pp = _write(tmp_path, "p.path", "s\tc0+ 100N c1+ 100N c2-\n")
    pairs = gapfill.read_path_file_pairs(pp, 20)
    with pytest.raises(KeyError):
        gapfill.choose_gap_reads(pairs, str(tmp_path / "ok.tsv"), _sequences({"c0": 1000, "c1": 1000}), argparse.Namespace(large_k=K), dev=dev)
    apart = text + "r1\tc0\t3\t10:+_20:+\n" + text
    with pytest.raises(ValueError, match="r0"):
        gapfill.choose_gap_reads(pairs, _write(tmp_path, "apart.tsv", apart), _sequences({"c0": 1000, "c1": 1000, "c2": 1000}),
                                 argparse.Namespace(large_k=K), dev=dev)
    dev.sync()


# ---------------------------------------------------------------- e. a pair table of chosen keys

GSEL_MULT = 0x9E3779B97F4A7C15
E_SLOTS, E_CTG, E_CTG_LEN = 64, 40, 20000
EMPTY_KEY = 0xFFFFFFFFFFFFFFFF


def gsel_slot(key, n_slots):
    """gsel_slot of csrc/gap_select_kernels.h: the slot a key's probe sequence starts at"""
    return (((key * GSEL_MULT) & EMPTY_KEY) >> 32) & (n_slots - 1)


def test_pair_table_source_literals():
    """cluster_case picks its pairs by gsel_slot above.  If the kernel's or the host's rule changes, the chosen clusters quietly turn
    into scattered keys: change the restatement with them."""
    squeezed = lambda name: re.sub(r"\s+", " ", open(os.path.join(os.path.dirname(HERE), "ntlink_amd", "csrc", name)).read())
    kernels, host = squeezed("gap_select_kernels.h"), squeezed("ntl_hip.hip")
    assert "uint64_t gsel_slot(uint64_t key, uint64_t n_slots) { return ((key * 0x%Xull) >> 32) & (n_slots - 1ull); }" % GSEL_MULT in kernels
    assert "uint64_t s = gsel_slot(key, A.n_slots);" in kernels and "s = (s + 1ull) & (A.n_slots - 1ull);" in kernels
    assert "if (have == key) return A.pair_vals[s]; if (have == GSEL_EMPTY) return GSEL_NONE;" in kernels
    assert "uint64_t s = gsel_slot(keys[i], n_slots); while (slot_keys[s] != GSEL_EMPTY) {" in host and "s = (s + 1) & (n_slots - 1);" in host
    assert "#define GSEL_EMPTY 0x%Xull" % EMPTY_KEY in kernels
    assert gsel_slot(0, 64) == 0 and gsel_slot(1, 64) == (GSEL_MULT >> 32) & 63 == 0x39 and gsel_slot(1 << 32, 1 << 32) == GSEL_MULT & 0xFFFFFFFF


def _node_name(node):
    return f"c{node >> 1}" + "+-"[node & 1]


def _revcomp_key(key):
    return (((key & 0xFFFFFFFF) ^ 1) << 32) | ((key >> 32) ^ 1)


def probe_table(keys, n_slots):
    """ntl_gap_pair_table in Python: (slot keys, slot values) of linear-probe inserts in the order of `keys`"""
    sk, sv = [EMPTY_KEY] * n_slots, [0] * n_slots
    for i, key in enumerate(keys):
        s = gsel_slot(key, n_slots)
        while sk[s] != EMPTY_KEY:
            s = (s + 1) & (n_slots - 1)
        sk[s], sv[s] = key, i
    return sk, sv


def first_empty(sk, s):
    while sk[s] != EMPTY_KEY:
        s = (s + 1) & (len(sk) - 1)
    return s


@functools.lru_cache(maxsize=None)
def cluster_case(seed=11):
    """(keys, verbose text, read kinds, an unused key): 40 contigs = 80 nodes, the 6240 keys of two nodes on different contigs
    enumerated by their home in a table of 64 slots.  32 pairs, none the reverse complement of another: 20 of home 62 (slots 62, 63,
    0 .. 17), 6 of home 30, one of home 3 (inside the cluster's run, which it lengthens to slot 18: the first empty slot behind it is 19), five of homes 40 .. 50.
    Reads: one per pair; one per reverse complement of every third pair; three each of absent pairs (absent as reverse complement
    too) of the homes 62, 63, 0, 17 -- inside the cluster, to be walked to slot 19 -- and 50; one of five mappings whose ten
    combinations hold present pairs, absent ones of a home inside the cluster and absent ones of an empty home."""
    rng = np.random.default_rng(seed)
    by_home = {}
    for s, t in itertools.product(range(2 * E_CTG), repeat=2):
        if s >> 1 != t >> 1:
            by_home.setdefault(gsel_slot((s << 32) | t, E_SLOTS), []).append((s << 32) | t)
    assert sum(len(v) for v in by_home.values()) == 6240 and len(by_home) == E_SLOTS
    keys = []

    def take(home, n):
        got = []
        for i in rng.permutation(len(by_home[home])):
            key = by_home[home][i]
            if key not in keys + got and _revcomp_key(key) not in keys + got:
                got.append(key)
                if len(got) == n:
                    return got
        raise AssertionError(home)

    for home, n in ((62, 20), (30, 6), (3, 1), (40, 1), (41, 1), (45, 1), (50, 2)):
        keys += take(home, n)
    keys = [keys[i] for i in rng.permutation(len(keys))]
    assert len(keys) == E_SLOTS // 2 == len(set(keys))
    present = set(keys)
    absent = lambda key: key not in present and _revcomp_key(key) not in present
    sk, _sv = probe_table(keys, E_SLOTS)
    occupied = {s for s in range(E_SLOTS) if sk[s] != EMPTY_KEY}
    assert occupied == {62, 63} | set(range(19)) | set(range(30, 36)) | {40, 41, 45, 50, 51}
    assert sorted(gsel_slot(sk[s], E_SLOTS) for s in [62, 63] + list(range(19))) == [3] + [62] * 20  # whichever of them lies where
    assert all(first_empty(sk, h) == 19 for h in (62, 63, 0, 17))

    reads = []  # (kind, [nodes in read order])
    for key in keys:
        reads.append(("present", [key >> 32, key & 0xFFFFFFFF]))
    for key in keys[::3]:
        rc = _revcomp_key(key)
        reads.append(("revcomp", [rc >> 32, rc & 0xFFFFFFFF]))
    for home in (62, 63, 0, 17, 50):
        got = [key for key in (by_home[home][i] for i in rng.permutation(len(by_home[home]))) if absent(key)][:3]
        assert len(got) == 3
        reads += [("absent", [key >> 32, key & 0xFFFFFFFF]) for key in got]
    unused = next(key for key in by_home[20] if absent(key))
    in_cluster = lambda key: gsel_slot(key, E_SLOTS) in occupied
    while True:  # five nodes on five contigs, two of them a pair of the cluster and two more a pair of home 30
        a, b = keys[int(rng.integers(0, len(keys)))], keys[int(rng.integers(0, len(keys)))]
        if gsel_slot(a, E_SLOTS) != 62 or gsel_slot(b, E_SLOTS) != 30:
            continue
        nodes = [a >> 32, b >> 32, int(rng.integers(0, 2 * E_CTG)), a & 0xFFFFFFFF, b & 0xFFFFFFFF]
        if len({n >> 1 for n in nodes}) < 5:
            continue
        tried = [(s << 32) | t for s, t in itertools.combinations(nodes, 2)]
        found = [key for key in tried if key in present or _revcomp_key(key) in present]
        missed = [key for key in tried if key not in present]
        if len(found) >= 2 and sum(1 for key in missed if in_cluster(key)) >= 2 and sum(1 for key in missed if not in_cluster(key)) >= 2:
            reads.append(("five", nodes))
            break
    rows, kinds = [], []
    for r, (kind, nodes) in enumerate(reads):
        kinds.append(kind)
        rpos = int(rng.integers(0, 3000))
        for node in nodes:
            toks, last = _hits(rng, (1, 2, 3, 65)[int(rng.integers(0, 4))], E_CTG_LEN, rpos, not node & 1, 0)
            rows.append(f"read{r}\tc{node >> 1}\t{int(rng.integers(1, 200))}\t{toks}")
            rpos = last + int(rng.integers(50, 4000))
    return keys, "".join(row + "\n" for row in rows), kinds, unused


def check_pair_clusters(dev, tmp_path):
    keys, verbose, kinds, unused = cluster_case()
    vp = _write(tmp_path, "e.verbose_mapping.tsv", verbose)
    ctg_names = [f"c{i}" for i in range(E_CTG)]
    ctg_len = np.full(E_CTG, E_CTG_LEN, np.uint32)
    sequences = _sequences({name: E_CTG_LEN for name in ctg_names})
    pairs = {(_node_name(key >> 32), _node_name(key & 0xFFFFFFFF)): None for key in keys}  # pair i is keys[i]
    assert len(pairs) == len(keys)
    # the host's table is the simulation's, slot for slot
    table = capi.pair_table(keys, n_slots=E_SLOTS, lib_path=dev.lib_path)
    sk, sv = probe_table(keys, E_SLOTS)
    assert table[0].tolist() == sk and table[1].tolist() == sv
    with pytest.raises(ValueError):  # 33 keys in 64 slots
        capi.pair_table(keys + [unused], n_slots=E_SLOTS, lib_path=dev.lib_path)
    # the restatement alone: what the comparison below relies on
    want, ids = gapfill.restated_candidates(pairs, vp, sequences, K)
    assert len(ids) == len(kinds)
    per_read = np.bincount(want["read"], minlength=len(kinds)).tolist()
    with open(vp) as fh:
        n_maps = [len(entries) for _rid, entries in formats.parse_verbose(fh)]
    tried = sum(n * (n - 1) // 2 for n in n_maps)
    assert 0 < len(want) < tried and n_maps[-1] == 5 and kinds[-1] == "five" and tried == len(kinds) - 1 + 10
    for r, kind in enumerate(kinds):
        mine = want[want["read"] == r]
        via = (mine["flags"] & capi.NTL_GAPSEL_VIA_REVCOMP) != 0
        if kind == "present":
            assert per_read[r] == 1 and mine["pair"][0] == r and not via[0]
        elif kind == "revcomp":
            assert per_read[r] == 1 and via[0] and gsel_slot(keys[int(mine["pair"][0])], E_SLOTS) in (62, 30, 3, 40, 41, 45, 50)
        elif kind == "absent":
            assert per_read[r] == 0
        else:
            assert 2 <= per_read[r] <= 6 and {gsel_slot(keys[int(p)], E_SLOTS) for p in mine["pair"]} >= {62, 30}
    assert sum(1 for kind in kinds if kind == "revcomp") == 11 and sum(1 for kind in kinds if kind == "absent") == 15
    # the device, the file whole and in blocks of a few reads
    for max_bytes in (0, SMALL_BLOCK):
        got, first = [], 0
        for block in formats.read_verbose(vp, ctg_names, max_bytes=max_bytes, lib_path=dev.lib_path):
            cands = dev.gap_select(block, ctg_len, K, table)
            cands["read"] += first
            first += len(block.names)
            got.append(cands)
        assert first == len(kinds) and (len(got) == 1 if not max_bytes else len(got) > 5)
        got = np.concatenate(got)
        assert len(got) == len(want), f"max_bytes {max_bytes}: {len(got)} candidates, the restated reference gives {len(want)}"
        for i in np.flatnonzero(got != want)[:5]:
            raise AssertionError(f"max_bytes {max_bytes}, record {i} (read {kinds[int(want[i]['read'])]}): {got[i]}, the restated reference gives {want[i]}")
    # one key more, put into the empty slot behind the cluster: more than half full, refused as in d.
    full = (table[0].copy(), table[1].copy())
    full[0][19], full[1][19] = unused, len(keys)
    (block,) = formats.read_verbose(vp, ctg_names, lib_path=dev.lib_path)
    with pytest.raises(capi.NtlError) as e:
        dev.gap_select(block, ctg_len, K, full)
    assert e.value.code == capi.NTL_EINVAL
    dev.sync()


# ---------------------------------------------------------------- under the SIMT mock

@pytest.fixture(scope="module")
def sim_dev():
    from sim import simlib
    dev = simlib.device()
    yield dev
    dev.close()


def test_sim_golden(sim_dev, tmp_path):
    check_golden(sim_dev, tmp_path, 0)


def test_sim_golden_in_blocks(sim_dev, tmp_path):
    check_golden(sim_dev, tmp_path, SMALL_BLOCK)


def test_sim_random(sim_dev, tmp_path):
    check_random(sim_dev, tmp_path)


def test_sim_reader(sim_dev, tmp_path, monkeypatch):
    check_reader(sim_dev.lib_path, tmp_path, monkeypatch)


def test_sim_reader_refusals(sim_dev, tmp_path):
    check_reader_refusals(sim_dev.lib_path, tmp_path)


def test_sim_refusals(sim_dev, tmp_path):
    check_refusals(sim_dev, tmp_path)


def test_sim_pair_clusters(sim_dev, tmp_path):
    check_pair_clusters(sim_dev, tmp_path)


# ---------------------------------------------------------------- on the GPU

@pytest.fixture(scope="module")
def gpu_dev():
    dev = capi.Device(0)
    yield dev
    dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("max_bytes", [0, SMALL_BLOCK])
def test_gpu_golden(gpu_dev, tmp_path, max_bytes):
    check_golden(gpu_dev, tmp_path, max_bytes)


@pytest.mark.gpu
def test_gpu_random(gpu_dev, tmp_path):
    check_random(gpu_dev, tmp_path)


@pytest.mark.gpu
def test_gpu_reader(gpu_dev, tmp_path, monkeypatch):
    check_reader(gpu_dev.lib_path, tmp_path, monkeypatch)


@pytest.mark.gpu
def test_gpu_reader_refusals(gpu_dev, tmp_path):
    check_reader_refusals(gpu_dev.lib_path, tmp_path)


@pytest.mark.gpu
def test_gpu_refusals(gpu_dev, tmp_path):
    check_refusals(gpu_dev, tmp_path)


@pytest.mark.gpu
def test_gpu_pair_clusters(gpu_dev, tmp_path):
    check_pair_clusters(gpu_dev, tmp_path)
