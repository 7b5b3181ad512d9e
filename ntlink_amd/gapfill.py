"""The gap filler's re-mapping loop in one device pass.

`map_long_reads` of the reference (bin/ntlink_patch_gaps.py:412-442) reads two temporary FASTA files in lockstep -- per gap one chosen
read piece and the two masked scaffold ends around the gap -- and per gap builds a minimizer dict of the two scaffold records alone
(read_btllib_minimizers, :397-410: a hash seen twice among the two is dropped), keeps the read's minimizers that are in it and calls
get_accepted_anchor_contigs.  Here all gaps of a batch are sketched together and mapped by ONE grouped call
(Device.map_grouped, ntl_map_run_grouped: gap g = group g, its contigs the records 2g and 2g+1, its read the record g):

    for gap in gapfill.map_gap_reads(scaffolds_fasta, reads_fasta, k, w, args):
        gap.read, gap.source, gap.target     # btllib-compatible records: .id .readlen .num (+ .minimizers with with_minimizers=True)
        gap.accepted, gap.order              # what get_accepted_anchor_contigs returns for this gap

* read record i belongs with the scaffold records 2i (source) and 2i+1 (target)
* the keys of ``accepted`` and ``ContigRun.contig`` are contig NAMES: ``name_of(record_id)``, by default the record id without its
  trailing ``_source`` / ``_target`` and without ``+`` / ``-`` at either end (what :415,426-433 make of it)
* a gap whose two names come out equal takes the single-index path (anchor.AnchorMapper), where the two records share one contig as
  they do in the reference's dict; the grouped call keeps two contigs apart
* contig lengths are the records' lengths: the reference's temporary files hold every scaffold N-masked to its full length
* ``args`` needs ``.k .z .x .sensitive``; ``MinimizerPositions.mx`` is the hash as ``str``

What the loop is for lies behind that call (:443-489): from the two accepted contigs the read's orientation on each scaffold, the
consistency of the positions, the terminal minimizer of each side and the cuts.  ``gap_cuts`` leaves all of it on the device
(MapResult.gap_cuts, ntl_mapres_gap_cuts, csrc/gap_kernels.h): per batch sketch, sketch, map_grouped, gap_cuts -- seven integers and a
status per gap come back, no hit and no sketch.  ``map_long_reads(pairs, scaffolds, args)`` is the drop-in for the reference function:
it reads the two temporary files of ``args.o`` and writes what :443-489 and fallback_old_anchor_cuts (:520-530) write into ``pairs``
and ``scaffolds``.

* a gap whose two names come out equal has ONE contig in the reference's dict, so ``len(accepted_anchor_contigs) != 2`` whatever
  maps: its status is NTL_GAP_NOT_TWO without any mapping (the grouped call, which keeps the two records apart, is overruled)

In front of all that stands the choice of every gap's read (:94-111, 149-198, 232-261, 311-342): ``read_path_file_pairs`` and
``choose_gap_reads(pairs, mappings_filename, sequences, args)``, the drop-in for read_verbose_mappings, choose_best_read_per_pair and
find_masking_cut_points in a row.  The verbose file is read block by block by the native reader (formats.read_verbose, ntl_vmap_*), one
device pass per block (Device.gap_select, ntl_gap_select, csrc/gap_select_kernels.h) returns a 32-byte record per (pair, supporting
read) and nothing else, and the host keeps per pair the running best: anchor sum descending, then read id descending as a string.
``choose_gap_reads_restated`` is the three reference functions restated over formats.parse_verbose; the tests and
tools/gapmap_bench.py compare against it, nothing falls back to it.

Between the two the reference writes and reads two temporary FASTA files (get_gap_fill_reads :264-273, print_masked_sequences :346-389):
per gap the whole source scaffold, the whole target scaffold and the whole read, N-masked but for the scaffold end beside the gap and
the read piece between its cuts.  ``get_gap_fill_reads`` / ``resident_scaffolds`` keep the chosen reads and the scaffolds on the device
instead, ``mask_ranges`` says what every record keeps, and ``gap_cuts_resident`` / ``map_long_reads_resident`` make the masked
full-length records there (Device.batch_mask, ntl_batch_mask, csrc/mask_kernels.h) and go on as the file form does: the same GapCuts,
the same fields in ``pairs`` and ``scaffolds``, the two files never written.  ``print_masked_sequences`` is the reference's function
restated over bytes for whoever wants the files; nothing falls back to it.

At the end stand the two functions the stage exists for (print_gap_filled_sequences :533-598 with :668-704, print_agp :600-665) and
main() (:760-836).  ``output_plan`` walks the path file ONCE and lists what both writers need: per output record its pieces (slices
of scaffolds and reads, runs of N), the AGP rows, the seven counters of the filling summary and the scaffolds no path names.
``print_gap_filled_sequences`` turns the pieces into segments of Device.stitch (ntl_stitch, csrc/stitch_kernels.h) over the bytes of
the scaffolds and the chosen reads, resident as they were read (Resident.ascii), and writes ``args.o`` from page-locked memory;
``print_agp`` writes ``args.o + ".agp"``; ``patch_gaps(args, dev)`` is main(): no temporary file is written, none is removed.
"""
import collections
import copy
import datetime
import itertools
import os
import re

import numpy as np

from . import anchor, capi, formats, seqio
from .anchor import ContigRun, Minimizer, MinimizerPositions

_STRAND = ("-", "+")
_LABEL = re.compile(r"_(source|target)$")
BATCH_BASES = 256 << 20  # bases of scaffold and read records per device pass (a gap is never split)


def default_name_of(record_id):
    """`scaf12+_source` -> `scaf12`"""
    return _LABEL.sub("", record_id).strip("+-")


class SketchMinimizer:
    """One minimizer of a record, with btllib's field names."""
    __slots__ = ("out_hash", "pos", "forward")

    def __init__(self, out_hash, pos, forward):
        self.out_hash, self.pos, self.forward = out_hash, pos, forward


class Record:
    """What btllib.Indexlr yields, as far as map_long_reads reads it."""
    __slots__ = ("id", "readlen", "num", "minimizers")

    def __init__(self, id, readlen, num, minimizers=None):
        self.id, self.readlen, self.num, self.minimizers = id, readlen, num, minimizers


class Gap:
    __slots__ = ("read", "source", "target", "accepted", "order")

    def __init__(self, read, source, target, accepted, order):
        self.read, self.source, self.target, self.accepted, self.order = read, source, target, accepted, order


class _Length:
    def __init__(self, length):
        self.length = length


def _minimizers(sk, i):
    off, h, p, s = sk
    a, b = int(off[i]), int(off[i + 1])
    return [SketchMinimizer(int(h[j]), int(p[j]), bool(s[j])) for j in range(a, b)]


def _single_index_gap(dev, ssk, rsk, g, name, ctg_len, read_len, args):
    """read_btllib_minimizers + get_accepted_anchor_contigs for a gap whose two records carry one contig name"""
    off, h, p, s = ssk
    mx_info, dup = {}, set()
    for j in range(int(off[2 * g]), int(off[2 * g + 2])):
        key = str(int(h[j]))
        if key in mx_info:
            dup.add(key)
        else:
            mx_info[key] = Minimizer(name, int(p[j]), _STRAND[int(s[j])])
    for key in dup:
        del mx_info[key]
    roff, rh, rp, rs = rsk
    mxs = [(str(int(rh[j])), int(rp[j]), _STRAND[int(rs[j])]) for j in range(int(roff[g]), int(roff[g + 1])) if str(int(rh[j])) in mx_info]
    return anchor.get_accepted_anchor_contigs(mxs, read_len, {name: _Length(ctg_len)}, mx_info, args, dev=dev)


def _map_batch(dev, scaffolds, reads, first, k, w, args, with_minimizers, name_of):
    """one device pass over len(reads) gaps; `first`: the number of the batch's first read record"""
    n = len(reads)
    names = [name_of(sid) for sid, _seq in scaffolds]
    equal = [g for g in range(n) if names[2 * g] == names[2 * g + 1]]
    ctg_len = np.fromiter((len(seq) for _id, seq in scaffolds), np.uint32, 2 * n)
    read_len = np.fromiter((len(seq) for _id, seq in reads), np.uint32, n)
    with dev.batch([bytes(seq) for _id, seq in scaffolds]) as sb, dev.batch([bytes(seq) for _id, seq in reads]) as rb, \
            dev.sketch(sb, k, w) as ssk, dev.sketch(rb, k, w) as rsk:
        with dev.map_grouped(ssk, ctg_len, 2 * np.arange(n + 1, dtype=np.uint32), rsk, read_len, np.arange(n + 1, dtype=np.uint32),
                             k=int(args.k), z=int(args.z), x=float(args.x), sensitive=bool(args.sensitive)) as res:
            rec = res.download()
        rmx = rsk.download()
        smx = ssk.download() if with_minimizers or equal else None
    maps, hits = rec["maps"], rec["hits"]
    # the hash of a hit: the read's record at that position (positions ascend within a read, reads are in order: one sorted key)
    roff, rh, rp, _rs = rmx
    read_of_mx = np.repeat(np.arange(n, dtype=np.uint64), np.diff(roff).astype(np.int64))
    mx_key = (read_of_mx << np.uint64(32)) | rp.astype(np.uint64)
    hit_read = np.repeat(maps["read"].astype(np.uint64), maps["n_hits"].astype(np.int64))
    where = np.searchsorted(mx_key, (hit_read << np.uint64(32)) | hits["read_pos"].astype(np.uint64))
    hit_hash = rh[where] if len(hits) else np.empty(0, np.uint64)
    accepted = [({}, []) for _ in range(n)]
    h_pos, h_rpos = hits["ctg_pos"].tolist(), hits["read_pos"].tolist()
    h_cs, h_rs, h_mx = hits["ctg_strand"].tolist(), hits["read_strand"].tolist(), hit_hash.tolist()
    for r, c, nh, ho in zip(maps["read"].tolist(), maps["ctg"].tolist(), maps["n_hits"].tolist(), maps["hit_off"].tolist()):
        name = names[c]
        run = ContigRun(name, [MinimizerPositions(mx=str(h_mx[j]), ctg_pos=h_pos[j], ctg_strand=_STRAND[h_cs[j]], read_pos=h_rpos[j],
                                                  read_strand=_STRAND[h_rs[j]]) for j in range(ho, ho + nh)])
        accepted[r][0][name] = run
        accepted[r][1].append(name)
    for g in equal:
        accepted[g] = _single_index_gap(dev, smx, rmx, g, names[2 * g], int(ctg_len[2 * g]), int(read_len[g]), args)
    for g in range(n):
        recs = [Record(reads[g][0], int(read_len[g]), first + g),
                Record(scaffolds[2 * g][0], int(ctg_len[2 * g]), 2 * (first + g)),
                Record(scaffolds[2 * g + 1][0], int(ctg_len[2 * g + 1]), 2 * (first + g) + 1)]
        if with_minimizers:
            recs[0].minimizers = _minimizers(rmx, g)
            recs[1].minimizers, recs[2].minimizers = _minimizers(smx, 2 * g), _minimizers(smx, 2 * g + 1)
        yield Gap(recs[0], recs[1], recs[2], accepted[g][0], accepted[g][1])


def _batches(scaffolds, reads, batch_bases):
    """scaffolds, reads: iterators of (id, sequence bytes); yields (number of the first read record, scaffold records, read records) of
    every batch: batches bounded by bases, a gap never split"""
    scaffolds, reads = iter(scaffolds), iter(reads)
    first, sb, rb, bases = 0, [], [], 0
    for read in reads:
        pair = [next(scaffolds, None), next(scaffolds, None)]
        if pair[1] is None:
            raise ValueError("fewer than two scaffold records per read record")
        add = len(read[1]) + len(pair[0][1]) + len(pair[1][1])
        if rb and bases + add > batch_bases:
            yield first, sb, rb
            first += len(rb)
            sb, rb, bases = [], [], 0
        rb.append(read); sb += pair; bases += add
    if next(scaffolds, None) is not None:
        raise ValueError("more than two scaffold records per read record")
    if rb:
        yield first, sb, rb


def _map_records(scaffolds, reads, k, w, args, dev, with_minimizers, name_of, batch_bases):
    dev = dev or anchor._default_device()
    for first, sb, rb in _batches(scaffolds, reads, batch_bases):
        yield from _map_batch(dev, sb, rb, first, k, w, args, with_minimizers, name_of)


def map_gap_sequences(scaffolds, reads, k, w, args, dev=None, with_minimizers=False, name_of=default_name_of, batch_bases=BATCH_BASES):
    """The in-memory form: scaffolds = [(id, sequence)] (two per gap: source, target), reads = [(id, sequence)]; sequences as bytes or
    str.  Yields one Gap per read record, in order."""
    scaffolds, reads = list(scaffolds), list(reads)
    if len(scaffolds) != 2 * len(reads):
        raise ValueError(f"{len(scaffolds)} scaffold records for {len(reads)} read records: two per read are needed")
    enc = lambda recs: ((i, s.encode() if isinstance(s, str) else s) for i, s in recs)
    return _map_records(enc(scaffolds), enc(reads), k, w, args, dev, with_minimizers, name_of, batch_bases)


# ---------------------------------------------------------------- the cuts (bin/ntlink_patch_gaps.py:443-489)

GapCuts = collections.namedtuple("GapCuts", "cuts read_ids scaffold_ids src_minus tgt_minus")
_READ_HEADER = re.compile(r"^(\S+)__(\S+)__(\S+)$")      # :414
_SCAFFOLD_HEADER = re.compile(r"^(\S+)_(source|target)$")  # :415


def _is_minus(record_id):
    """the sign :426-433 take from a scaffold record: the character in front of `_source` / `_target`"""
    sign = _LABEL.sub("", record_id)[-1:]
    if sign not in ("+", "-"):
        raise ValueError(f"scaffold record {record_id!r}: + or - is needed in front of _source / _target")
    return sign == "-"


def _cut_device(dev, sb, rb, ctg_len, read_len, src_minus, tgt_minus, k, w, args):
    """sketch, sketch, map_grouped, gap_cuts over the resident batches sb (two records per gap) and rb (one per gap)"""
    n = len(read_len)
    with dev.sketch(sb, k, w) as ssk, dev.sketch(rb, k, w) as rsk, \
            dev.map_grouped(ssk, ctg_len, 2 * np.arange(n + 1, dtype=np.uint32), rsk, read_len, np.arange(n + 1, dtype=np.uint32),
                            k=int(args.k), z=int(args.z), x=float(args.x), sensitive=bool(args.sensitive)) as res:
        return res.gap_cuts(src_minus, tgt_minus, int(args.k))


def _cut_batch(dev, scaffolds, reads, k, w, args, name_of):
    """one device pass over len(reads) gaps: sketch, sketch, map_grouped, gap_cuts; nothing but the cut records comes back"""
    n = len(reads)
    src_minus = np.fromiter((_is_minus(scaffolds[2 * g][0]) for g in range(n)), np.uint8, n)
    tgt_minus = np.fromiter((_is_minus(scaffolds[2 * g + 1][0]) for g in range(n)), np.uint8, n)
    ctg_len = np.fromiter((len(seq) for _id, seq in scaffolds), np.uint32, 2 * n)
    read_len = np.fromiter((len(seq) for _id, seq in reads), np.uint32, n)
    with dev.batch([bytes(seq) for _id, seq in scaffolds]) as sb, dev.batch([bytes(seq) for _id, seq in reads]) as rb:
        cuts = _cut_device(dev, sb, rb, ctg_len, read_len, src_minus, tgt_minus, k, w, args)
    for g in range(n):  # one contig in the reference's dict: never two accepted contigs (see the module's text)
        if name_of(scaffolds[2 * g][0]) == name_of(scaffolds[2 * g + 1][0]):
            cuts[g] = (capi.NTL_GAP_NOT_TWO, 0, 0, 0, 0, 0, 0, 0)
    return cuts, src_minus, tgt_minus


def _cut_records(scaffolds, reads, k, w, args, dev, name_of, batch_bases):
    dev = dev or anchor._default_device()
    parts, rids, sids = [], [], []
    for _first, sb, rb in _batches(scaffolds, reads, batch_bases):
        parts.append(_cut_batch(dev, sb, rb, k, w, args, name_of))
        rids += [rid for rid, _seq in rb]
        sids += [sid for sid, _seq in sb]
    cat = lambda i, dt: np.concatenate([p[i] for p in parts]) if parts else np.empty(0, dt)
    return GapCuts(cat(0, capi.GAP_CUT_DT), rids, sids, cat(1, np.uint8), cat(2, np.uint8))


def gap_cut_sequences(scaffolds, reads, k, w, args, dev=None, name_of=default_name_of, batch_bases=BATCH_BASES):
    """gap_cuts over records in memory, as map_gap_sequences takes them"""
    scaffolds, reads = list(scaffolds), list(reads)
    if len(scaffolds) != 2 * len(reads):
        raise ValueError(f"{len(scaffolds)} scaffold records for {len(reads)} read records: two per read are needed")
    enc = lambda recs: ((i, s.encode() if isinstance(s, str) else s) for i, s in recs)
    return _cut_records(enc(scaffolds), enc(reads), k, w, args, dev, name_of, batch_bases)


def gap_cuts(scaffolds_fasta, reads_fasta, k, w, args, dev=None, name_of=default_name_of, batch_bases=BATCH_BASES):
    """The cuts of every gap of the two temporary files, decided on the device: GapCuts(cuts, read_ids, scaffold_ids, src_minus,
    tgt_minus) -- cuts: one capi.GAP_CUT_DT record per read record, in file order (status 0: valid; else NTL_GAP_* bits and zeros);
    src_minus / tgt_minus: 1 where the scaffold record's sign is '-'.  Batches as map_gap_reads makes them."""
    return _cut_records(_records_of(scaffolds_fasta, batch_bases), _records_of(reads_fasta, batch_bases), k, w, args, dev, name_of,
                        batch_bases)


def _fallback_old_anchor_cuts(pair, scaffolds, source_name, src_minus, target_name, tgt_minus):
    """fallback_old_anchor_cuts (:520-530)"""
    pair.old_anchor_used = True
    if not src_minus:
        scaffolds[source_name].three_prime_cut = pair.source_ctg_cut
    else:
        scaffolds[source_name].five_prime_cut = pair.source_ctg_cut
    if not tgt_minus:
        scaffolds[target_name].five_prime_cut = pair.target_ctg_cut
    else:
        scaffolds[target_name].three_prime_cut = pair.target_ctg_cut


def _apply_cut(pair, scaffolds, args, source_name, src_minus, target_name, tgt_minus, cut):
    """what :443-489 write for one gap: `cut` is its capi.GAP_CUT_DT record as a tuple"""
    status, src_pos, src_read_cut, src_end_cut, tgt_pos, tgt_read_cut, tgt_end_cut, _ori = cut
    if status:  # not two accepted contigs, mixed strands or inconsistent positions (:443-463)
        if args.stringent:
            pair.source_read_cut = None
            pair.target_read_cut = None
        else:
            _fallback_old_anchor_cuts(pair, scaffolds, source_name, src_minus, target_name, tgt_minus)
        return
    pair.source_ctg_cut, pair.source_read_cut = src_pos, src_read_cut
    if not src_minus:
        scaffolds[source_name].three_prime_cut = src_end_cut
    else:
        scaffolds[source_name].five_prime_cut = src_end_cut
    pair.target_ctg_cut, pair.target_read_cut = tgt_pos, tgt_read_cut
    if not tgt_minus:
        scaffolds[target_name].five_prime_cut = tgt_end_cut
    else:
        scaffolds[target_name].three_prime_cut = tgt_end_cut


def map_long_reads(pairs, scaffolds, args, dev=None, batch_bases=BATCH_BASES):
    """The reference's map_long_reads (:412-489): reads ``args.o + ".scaffolds.masked_temp.fa"`` / ``".reads.masked_temp.fa"``, uses
    ``args.k .w .z .x .sensitive .stringent`` and writes ``pairs[(source, target)].source_ctg_cut / source_read_cut / target_ctg_cut /
    target_read_cut / old_anchor_used`` and ``scaffolds[name].five_prime_cut / three_prime_cut``.  Gaps are applied in file order: a
    scaffold can be the source of one gap and the target of another."""
    got = gap_cuts(args.o + ".scaffolds.masked_temp.fa", args.o + ".reads.masked_temp.fa", int(args.k), int(args.w), args, dev=dev,
                   batch_bases=batch_bases)
    for g, cut in enumerate(got.cuts.tolist()):
        _, source, target = _READ_HEADER.search(got.read_ids[g]).groups()
        source_id, label = _SCAFFOLD_HEADER.search(got.scaffold_ids[2 * g]).groups()
        assert source_id == source and label == "source"
        target_id, label = _SCAFFOLD_HEADER.search(got.scaffold_ids[2 * g + 1]).groups()
        assert target_id == target and label == "target"
        _apply_cut(pairs[(source, target)], scaffolds, args, source_id.strip("+-"), bool(got.src_minus[g]), target_id.strip("+-"),
                   bool(got.tgt_minus[g]), cut)


def _records_of(path, batch_bases):
    for ss in seqio.load(path, max_bases=batch_bases):
        off = ss.offsets.tolist()
        for i, name in enumerate(ss.names):
            yield name, ss.buf[off[i]:off[i + 1]]


def map_gap_reads(scaffolds_fasta, reads_fasta, k, w, args, dev=None, with_minimizers=False, name_of=default_name_of,
                  batch_bases=BATCH_BASES):
    """The loop header of map_long_reads over its two temporary files (<o>.scaffolds.masked_temp.fa, <o>.reads.masked_temp.fa).
    A scaffold count other than twice the read count raises ValueError."""
    return _map_records(_records_of(scaffolds_fasta, batch_bases), _records_of(reads_fasta, batch_bases), k, w, args, dev,
                        with_minimizers, name_of, batch_bases)


# ---------------------------------------------------------------- without the two temporary files (bin/ntlink_patch_gaps.py:264-273, 346-389)

class Resident:
    """Records resident on the device: ``ids``, ``lengths`` (u32), ``number`` (id -> record number) and ``batch`` (capi.Batch).  With
    keep_ascii also the bytes as they were read, case and IUPAC codes included (``buf``, ``offsets``; ``resident[id]`` is one
    record's).  With stitchable the same bytes are resident too (``ascii``: capi.Ascii, a source of Device.stitch).  Close it, or use
    it as a context manager, to free the batch and the bytes."""

    def __init__(self, ids, lengths, batch, buf=None, offsets=None, ascii=None):
        self.ids, self.lengths, self.batch, self.buf, self.offsets = list(ids), np.ascontiguousarray(lengths, np.uint32), batch, buf, offsets
        self.ascii = ascii
        self.number = {rid: i for i, rid in enumerate(self.ids)}
        if len(self.number) != len(self.ids):
            raise ValueError("two records with the same id")

    def __len__(self):
        return len(self.ids)

    def __contains__(self, rid):
        return rid in self.number

    def __getitem__(self, rid):
        if self.buf is None:
            raise ValueError("the records' bytes were not kept (keep_ascii=True keeps them)")
        i = self.number[rid]
        return bytes(self.buf[int(self.offsets[i]):int(self.offsets[i + 1])])

    def length_of(self):
        return dict(zip(self.ids, self.lengths.tolist()))

    def close(self):
        if self.batch is not None:
            self.batch.close()
            self.batch = None
        if self.ascii is not None:
            self.ascii.close()
            self.ascii = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def _resident(dev, ids, seqs, keep_ascii, stitchable=False):
    lens = np.fromiter((len(s) for s in seqs), np.uint64, len(seqs))
    offsets = np.zeros(len(seqs) + 1, np.uint64)
    np.cumsum(lens, out=offsets[1:])
    buf = np.frombuffer(b"".join(seqs), np.uint8)
    batch = dev.batch(buf, offsets)
    return Resident(ids, lens, batch, buf if keep_ascii else None, offsets if keep_ascii else None,
                    dev.ascii(buf, offsets) if stitchable else None)


def get_gap_fill_reads(reads_filename_list, pairs, args=None, dev=None, keep_ascii=False, max_bases=BATCH_BASES, stitchable=False):
    """get_gap_fill_reads (:264-273): goes through the read files (FASTA / FASTQ, gzip or not) and keeps the chosen reads of `pairs`
    only -- as ONE resident batch instead of a dict of strings.  A later record with the same id replaces an earlier one, as the
    reference's dict does (and keeps the earlier one's place).  -> Resident.  `args` is not read (the reference takes its thread
    count from it)."""
    dev = dev or anchor._default_device()
    wanted = {p.chosen_read for p in pairs.values() if p.chosen_read is not None}
    kept = {}
    for ss in seqio.load(list(reads_filename_list), max_bases=max_bases):
        off = ss.offsets.tolist()
        for i, name in enumerate(ss.names):
            if name in wanted:
                kept[name] = bytes(ss.buf[off[i]:off[i + 1]])
    return _resident(dev, list(kept), list(kept.values()), keep_ascii, stitchable)


def resident_scaffolds(path_or_records, dev=None, keep_ascii=False, stitchable=False):
    """The scaffolds of ``args.s`` as one resident batch: a FASTA path, or records [(id, sequence as bytes or str)].  -> Resident.
    One batch holds up to 2^32 - 4112 bases."""
    dev = dev or anchor._default_device()
    if isinstance(path_or_records, str):
        ss = seqio.load_all([path_or_records])
        return Resident(ss.names.tolist(), ss.lengths, dev.batch(ss.buf, ss.offsets), ss.buf if keep_ascii else None,
                        ss.offsets if keep_ascii else None, dev.ascii(ss.buf, ss.offsets) if stitchable else None)
    recs = [(rid, seq.encode() if isinstance(seq, str) else bytes(seq)) for rid, seq in path_or_records]
    return _resident(dev, [rid for rid, _seq in recs], [seq for _rid, seq in recs], keep_ascii, stitchable)


MaskRanges = collections.namedtuple("MaskRanges", "keys scaffold_names scaffold_lo scaffold_hi read_ids read_lo read_hi src_minus tgt_minus")


def mask_ranges(pairs, scaffold_lengths, read_lengths):
    """What print_masked_sequences keeps of every record it writes (:351-386), as half-open ranges.  Pairs in dict order, pairs
    without a chosen read skipped.  -> MaskRanges: per gap g its key (source, target), scaffold_names[2g], [2g+1] and the ranges
    scaffold_lo/hi[2g], [2g+1] (source +: [cut, len), source -: [0, cut), target +: [0, cut), target -: [cut, len)), the read's id
    and its range [min, max) of the two read cuts, and the two signs (1: '-').  scaffold_lengths: name -> length; read_lengths:
    read id -> length.  ValueError for a node that does not end in + or - (the reference's) and for a cut beyond its sequence, where
    Python's slices would silently make the record longer."""
    keys, names, read_ids, slo, shi, rlo, rhi, sm, tm = [], [], [], [], [], [], [], [], []
    for (source, target), info in pairs.items():
        if info.chosen_read is None:
            continue
        for node, cut, is_source in ((source, info.source_ctg_cut, True), (target, info.target_ctg_cut, False)):
            if node[-1:] not in ("+", "-"):
                raise ValueError(f"{node[-1:]} must be + or -")
            name, minus = node.strip("+-"), node[-1] == "-"
            length = int(scaffold_lengths[name])
            if not 0 <= cut <= length:
                raise ValueError(f"pair {source} {target}: cut {cut} outside {name}'s {length} bases")
            tail = minus != is_source  # source +, target -: the end behind the cut is kept
            slo.append(cut if tail else 0)
            shi.append(length if tail else cut)
            names.append(name)
            (sm if is_source else tm).append(minus)
        a, b = sorted((info.source_read_cut, info.target_read_cut))
        length = int(read_lengths[info.chosen_read])
        if not 0 <= a <= b <= length:
            raise ValueError(f"pair {source} {target}: read cuts {a}, {b} outside {info.chosen_read}'s {length} bases")
        keys.append((source, target)); read_ids.append(info.chosen_read); rlo.append(a); rhi.append(b)
    u32 = lambda v: np.array(v, np.uint32)
    return MaskRanges(keys, names, u32(slo), u32(shi), read_ids, u32(rlo), u32(rhi), np.array(sm, np.uint8), np.array(tm, np.uint8))


def gap_cuts_resident(pairs, scaffolds, reads, k, w, args, dev=None, batch_bases=BATCH_BASES):
    """gap_cuts without the two files: the same GapCuts as gap_cuts over what print_masked_sequences would write for `pairs`.
    scaffolds, reads: Resident (resident_scaffolds, get_gap_fill_reads).  Gaps are batched as the file form batches them -- by the full
    lengths of their three records, a gap never split -- and per batch two Device.batch_mask calls make the masked records on the
    device (csrc/mask_kernels.h); then sketch, sketch, map_grouped, gap_cuts as ever."""
    dev = dev or anchor._default_device()
    r = mask_ranges(pairs, scaffolds.length_of(), reads.length_of())
    n = len(r.keys)
    snum = np.fromiter((scaffolds.number[name] for name in r.scaffold_names), np.uint32, 2 * n)
    rnum = np.fromiter((reads.number[rid] for rid in r.read_ids), np.uint32, n)
    ctg_len, read_len = scaffolds.lengths[snum], reads.lengths[rnum]
    per_gap = (read_len.astype(np.int64) + ctg_len[0::2] + ctg_len[1::2]).tolist()
    bounds, bases = [0], 0
    for g, add in enumerate(per_gap):
        if g > bounds[-1] and bases + add > batch_bases:
            bounds.append(g)
            bases = 0
        bases += add
    bounds.append(n)
    cuts = np.zeros(n, capi.GAP_CUT_DT)
    for a, b in zip(bounds, bounds[1:]):
        if a == b:
            continue
        with dev.batch_mask(scaffolds.batch, snum[2 * a:2 * b], r.scaffold_lo[2 * a:2 * b], r.scaffold_hi[2 * a:2 * b]) as sb, \
                dev.batch_mask(reads.batch, rnum[a:b], r.read_lo[a:b], r.read_hi[a:b]) as rb:
            cuts[a:b] = _cut_device(dev, sb, rb, ctg_len[2 * a:2 * b], read_len[a:b], r.src_minus[a:b], r.tgt_minus[a:b], k, w, args)
    for g in range(n):  # one contig in the reference's dict: never two accepted contigs (see the module's text)
        if r.scaffold_names[2 * g] == r.scaffold_names[2 * g + 1]:
            cuts[g] = (capi.NTL_GAP_NOT_TWO, 0, 0, 0, 0, 0, 0, 0)
    read_ids = [f"{rid}__{source}__{target}" for rid, (source, target) in zip(r.read_ids, r.keys)]
    scaffold_ids = [sid for source, target in r.keys for sid in (source + "_source", target + "_target")]
    return GapCuts(cuts, read_ids, scaffold_ids, r.src_minus, r.tgt_minus)


def map_long_reads_resident(pairs, sequences, scaffolds, reads, args, dev=None, batch_bases=BATCH_BASES):
    """map_long_reads without the two files: writes into ``pairs`` and ``sequences`` (name -> object with ``five_prime_cut``,
    ``three_prime_cut``) exactly what map_long_reads writes after print_masked_sequences.  scaffolds, reads: Resident.  Source, target
    and the signs come from the keys of ``pairs``, not from record headers."""
    got = gap_cuts_resident(pairs, scaffolds, reads, int(args.k), int(args.w), args, dev=dev, batch_bases=batch_bases)
    keys = [key for key, info in pairs.items() if info.chosen_read is not None]
    for g, (cut, (source, target)) in enumerate(zip(got.cuts.tolist(), keys)):
        _apply_cut(pairs[(source, target)], sequences, args, source.strip("+-"), bool(got.src_minus[g]), target.strip("+-"),
                   bool(got.tgt_minus[g]), cut)


def print_masked_sequences(scaffolds, reads, pairs, args):
    """print_masked_sequences (:346-389) restated over bytes: writes ``args.o + ".scaffolds.masked_temp.fa"`` and
    ``".reads.masked_temp.fa"``, byte for byte the reference's.  scaffolds: name -> sequence, or -> object with ``.seq``; reads: id ->
    sequence (str or bytes; a Resident made with keep_ascii serves as either).  For whoever wants the two files and for
    tools/gapmap_bench.py's file leg; nothing falls back to it."""
    def seq_of(rec):
        rec = getattr(rec, "seq", rec)
        return rec.encode() if isinstance(rec, str) else rec

    with open(args.o + ".scaffolds.masked_temp.fa", "wb") as out_scaffolds, open(args.o + ".reads.masked_temp.fa", "wb") as out_reads:
        for (source, target), info in pairs.items():
            if info.chosen_read is None:
                continue
            for node, cut, label, tail_on in ((source, info.source_ctg_cut, b"_source", "+"), (target, info.target_ctg_cut, b"_target", "-")):
                if node[-1:] not in ("+", "-"):
                    raise ValueError(f"{node[-1:]} must be + or -")
                seq = seq_of(scaffolds[node.strip("+-")])
                if node[-1] == tail_on:
                    body = b"N" * cut + seq[cut:]
                else:
                    body = seq[:cut] + b"N" * (len(seq) - cut)
                out_scaffolds.write(b">" + node.encode() + label + b"\n" + body + b"\n")
            start, end = sorted((info.source_read_cut, info.target_read_cut))
            seq = seq_of(reads[info.chosen_read])
            out_reads.write(b">" + f"{info.chosen_read}__{source}__{target}".encode() + b"\n" + b"N" * start + seq[start:end] +
                            b"N" * (len(seq) - end) + b"\n")


# ---------------------------------------------------------------- the read of every gap (bin/ntlink_patch_gaps.py:94-111, 149-261, 311-342)

VERBOSE_BLOCK_BYTES = 64 << 20  # text per device pass of choose_gap_reads (a read's lines are never split)
_GAP = re.compile(r"^(\d+)N$")  # :97


class PairInfo:
    """A pair of the path file with the reference's fields (:55-65)"""

    def __init__(self, gap_size):
        self.gap_size = int(gap_size)
        self.mapping_reads = set()
        self.chosen_read = None
        self.source_ctg_cut = None
        self.source_read_cut = None
        self.target_ctg_cut = None
        self.target_read_cut = None
        self.old_anchor_used = False
        self.chosen_reversed = None  # the chosen read lies on the source the other way round than the path has it (:567, :636)


def read_path_file_pairs(path_filename, min_gap_size):
    """read_path_file_pairs (:94-111): (source node, target node) -> PairInfo for every `<n>N` between two nodes with n > min_gap_size;
    abyss-scaffold's gap is one more than the estimate"""
    pairs = {}
    with open(path_filename, "r") as fin:
        for line in fin:
            line = line.strip().split("\t")
            if len(line) < 2:
                continue
            _, path = line
            path = path.split(" ")
            for idx in range(len(path) - 2):
                i, j, k = path[idx:idx + 3]
                gap_match = _GAP.search(j)
                if gap_match and int(gap_match.group(1)) > min_gap_size:
                    pairs[(i, k)] = PairInfo(int(gap_match.group(1)) - 1)
    return pairs


def _node(node):
    if node[-1:] not in ("+", "-"):
        raise ValueError("+ or - needed for last character of node, found " + node[-1:])  # reverse_complement_pair (:130-146)
    return node[:-1], node[-1] == "-"


def pair_tables(pairs, sequences):
    """What the device pass needs of the path's pairs: (contig names, ctg_len u32, keys u64) -- the contigs the pairs name, in order of
    first appearance, and per pair its key in ntl_gap_select's table.  KeyError for a contig that is not in `sequences`."""
    number, names, lengths, keys = {}, [], [], []
    for source, target in pairs:
        nodes = []
        for node in (source, target):
            name, minus = _node(node)
            if name not in number:
                number[name] = len(names)
                names.append(name)
                lengths.append(int(sequences[name].length))
            nodes.append((number[name], minus))
        keys.append(capi.pair_key(nodes[0][0], nodes[0][1], nodes[1][0], nodes[1][1]))
    return names, np.array(lengths, np.uint32), np.array(keys, np.uint64)


def gap_candidates(mappings_filename, ctg_names, ctg_len, keys, large_k, dev=None, max_bytes=VERBOSE_BLOCK_BYTES):
    """Per block of the verbose file: (VerboseBlock, capi.GAP_CAND_DT records) -- every (pair, supporting read) of the block with its
    anchor sum, flags and the cuts the read would give."""
    dev = dev or anchor._default_device()
    table = capi.pair_table(keys, lib_path=dev.lib_path)
    for block in formats.read_verbose(mappings_filename, ctg_names, max_bytes=max_bytes, lib_path=dev.lib_path):
        yield block, dev.gap_select(block, ctg_len, large_k, table)


def choose_gap_reads(pairs, mappings_filename, sequences, args, dev=None, max_bytes=VERBOSE_BLOCK_BYTES):
    """read_verbose_mappings, choose_best_read_per_pair and find_masking_cut_points of the reference in a row (:178-198, 249-261,
    311-342): fills ``mapping_reads`` of every pair and sets ``chosen_read`` and the four cuts of every pair that has a valid supporting
    read.  pairs: what read_path_file_pairs returns; sequences: name -> object with ``.length``; args: ``.large_k``.

    * KeyError, before anything is read, for a pair whose contig is not in ``sequences``
    * AssertionError where the reference's ``assert a >= 0`` / ``assert b >= 0`` (:222-223) fails on a read it reaches: a pair whose
      best read among the valid and the negative ones is a negative one
    * ValueError for a read id that supports pairs from two separate groups of lines (the reference overwrites the first silently),
      and for a malformed line (with its number)"""
    ctg_names, ctg_len, keys = pair_tables(pairs, sequences)
    infos = list(pairs.values())
    best = [None] * len(infos)  # per pair (anchor sum, read id, negative, the four cuts) of the first read the reference would stop at
    seen = {}                   # read id -> (block, read) among the reads that gave a candidate
    stop = capi.NTL_GAPSEL_VALID | capi.NTL_GAPSEL_NEGATIVE
    for b, (block, cands) in enumerate(gap_candidates(mappings_filename, ctg_names, ctg_len, keys, int(args.large_k), dev, max_bytes)):
        if not len(cands):
            continue
        raw, off = block.names.blob.tobytes(), block.names.off
        ids = {}
        for pair, read, anchors, flags, sc, sr, tc, tr in cands.tolist():
            rid = ids.get(read)
            if rid is None:
                rid = ids[read] = raw[int(off[read]):int(off[read + 1])].decode()
                if seen.setdefault(rid, (b, read)) != (b, read):
                    raise ValueError(f"{mappings_filename}: read {rid} supports pairs from two separate groups of lines")
            infos[pair].mapping_reads.add(rid)
            if flags & stop and (best[pair] is None or (anchors, rid) > best[pair][:2]):
                best[pair] = (anchors, rid, bool(flags & capi.NTL_GAPSEL_NEGATIVE), sc, sr, tc, tr, bool(flags & capi.NTL_GAPSEL_VIA_REVCOMP))
    for (source, target), info, got in zip(pairs, infos, best):
        if got is None:
            continue
        assert not got[2], f"pair {source} {target}, read {got[1]}: a negative distance to a contig end (calculate_est_gap_size)"
        info.chosen_read = got[1]
        info.source_ctg_cut, info.source_read_cut, info.target_ctg_cut, info.target_read_cut = got[3:7]
        info.chosen_reversed = got[7]  # found directly: the read has the source's sign; as the reverse-complement pair: the other


# The same in plain Python, as the reference has it: the comparison for the tests and for tools/gapmap_bench.py, never a fallback.

def _reverse_complement_pair(source, target):
    """:130-146"""
    flip = {"+": "-", "-": "+"}
    return target[:-1] + flip[target[-1]], source[:-1] + flip[source[-1]]


def _restated_mappings(mappings_filename):
    """per read of the file (id, mapping dict, mapping order) as tally_contig_mapping_info builds them (:149-163): contig -> (anchors,
    hits, orientation) of the valid mappings and "length" """
    with open(mappings_filename) as fh:
        for read_id, entries in formats.parse_verbose(fh, with_anchors=True):
            info, order = {}, []
            for ctg, hits, anchors in entries:
                if all(h[1] == h[3] for h in hits):
                    orientation = "+"
                elif all(h[1] != h[3] for h in hits):
                    orientation = "-"
                else:
                    continue
                if not (all(a[0] < b[0] for a, b in zip(hits, hits[1:])) or all(a[0] > b[0] for a, b in zip(hits, hits[1:]))):
                    continue
                info[ctg] = (anchors, hits, orientation)
                order.append(ctg + orientation)
                info["length"] = hits[-1][2]
            yield read_id, info, order


def _restated_valid(source, target, info, sequences, k):
    """is_valid_supporting_read with calculate_est_gap_size (:208-246) -> (valid, negative); the reference asserts where negative"""
    if source[-1] != info[source[:-1]][2]:
        assert target[-1] != info[target[:-1]][2]
        source, target = _reverse_complement_pair(source, target)
    s_mx, t_mx = info[source[:-1]][1][-1], info[target[:-1]][1][0]
    a = sequences[source[:-1]].length - s_mx[0] - k if source[-1] == "+" else s_mx[0]
    b = t_mx[0] if target[-1] == "+" else sequences[target[:-1]].length - t_mx[0] - k
    return abs(t_mx[2] - s_mx[2] - a - b) <= info["length"], a < 0 or b < 0


def _restated_cuts(source, target, info, k):
    """find_masking_cut_points for one pair and one read (:317-342)"""
    _sa, s_hits, s_ori = info[source[:-1]]
    _ta, t_hits, t_ori = info[target[:-1]]
    s_mx = s_hits[-1] if s_ori == source[-1] else s_hits[0]
    t_mx = t_hits[0] if t_ori == target[-1] else t_hits[-1]
    ctg_cut = lambda pos, ori, sign: pos + k if ori == sign and sign == "-" else pos   # assign_ctg_cut (:291-299)
    read_cut = lambda pos, ori, sign: pos + k if ori != sign and sign == "+" else pos  # assign_read_cut (:301-308)
    return (ctg_cut(s_mx[0], s_ori, source[-1]), read_cut(s_mx[2], s_ori, source[-1]),
            ctg_cut(t_mx[0], t_ori, target[-1]), read_cut(t_mx[2], t_ori, target[-1]))


def restated_candidates(pairs, mappings_filename, sequences, large_k):
    """The records ntl_gap_select must return for the whole file as one block (capi.GAP_CAND_DT; `read` counts the file's reads), and
    the reads' ids"""
    number = {pair: i for i, pair in enumerate(pairs)}
    out, ids = [], []
    for r, (read_id, info, order) in enumerate(_restated_mappings(mappings_filename)):
        ids.append(read_id)
        for i, j in itertools.combinations(order, 2):
            for pair, via in (((i, j), 0), (_reverse_complement_pair(i, j), capi.NTL_GAPSEL_VIA_REVCOMP)):
                if pair in number:
                    valid, negative = _restated_valid(pair[0], pair[1], info, sequences, large_k)
                    out.append((number[pair], r, info[pair[0][:-1]][0] + info[pair[1][:-1]][0],
                                int(valid) | (capi.NTL_GAPSEL_NEGATIVE if negative else 0) | via, *_restated_cuts(pair[0], pair[1], info, large_k)))
    return np.array(out, capi.GAP_CAND_DT), ids


def choose_gap_reads_restated(pairs, mappings_filename, sequences, args):
    """read_verbose_mappings, choose_best_read_per_pair and find_masking_cut_points (:178-198, 249-261, 311-342), dicts and all"""
    mappings = {}
    for read_id, info, order in _restated_mappings(mappings_filename):
        added = False
        for i, j in itertools.combinations(order, 2):
            for pair in ((i, j), _reverse_complement_pair(i, j)):
                if pair in pairs:
                    pairs[pair].mapping_reads.add(read_id)
                    added = True
        if added:
            mappings[read_id] = info
    for (source, target), pair in pairs.items():
        reads = [(read_id, mappings[read_id][source.strip("+-")][0], mappings[read_id][target.strip("+-")][0]) for read_id in pair.mapping_reads]
        for read_id, _, _ in sorted(reads, key=lambda x: (np.mean([x[1], x[2]]), x[0]), reverse=True):
            valid, negative = _restated_valid(source, target, mappings[read_id], sequences, args.large_k)
            assert not negative
            if valid:
                pair.chosen_read = read_id
                pair.chosen_reversed = mappings[read_id][source.strip("+-")][2] != source[-1]
                break
    for (source, target), pair in pairs.items():
        if pair.chosen_read is not None:
            pair.source_ctg_cut, pair.source_read_cut, pair.target_ctg_cut, pair.target_read_cut = \
                _restated_cuts(source, target, mappings[pair.chosen_read], args.large_k)


# ---------------------------------------------------------------- the output (bin/ntlink_patch_gaps.py:20-45, 533-713, 733-836)

STITCH_BYTES = 1 << 30   # output text per Device.stitch call (whole records; a larger record goes alone)
WRITE_PIECE = 64 << 20   # bytes per copy into page-locked memory and ntl_write_blob
_COUNTERS = ("num_gaps", "overlap_pts", "small_gaps", "potential_fills", "filled_gaps", "new_anchor_used", "old_anchor_used")


class ScaffoldGaps:
    """A scaffold with the reference's fields (:20-45).  ``seq`` may stay None: the stage keeps the bytes on the device."""

    def __init__(self, seq=None, length=None):
        self.seq = seq
        self.length = len(seq) if length is None else int(length)
        self.five_prime_cut = 0
        self.three_prime_cut = self.length
        self.five_prime_trim = 0
        self.three_prime_trim = self.length

    def get_cut_coordinates(self):
        return max(self.five_prime_trim, self.five_prime_cut), min(self.three_prime_trim, self.three_prime_cut)


def read_trim_coordinates(sequences, args):
    """read_trim_coordinates (:707-713)"""
    with open(args.trims, "r") as fin:
        for line in fin:
            ctg, start, end = line.strip().split("\t")
            sequences[ctg].five_prime_trim = int(start)
            sequences[ctg].three_prime_trim = int(end)


OutputPlan = collections.namedtuple("OutputPlan", "records agp counters printed unassigned")


def _slice(lo, hi, length):
    """[lo, hi) as Python's slice of a sequence of `length` takes it (lo, hi >= 0): clamped, empty where they cross"""
    lo, hi = min(lo, length), min(hi, length)
    return (lo, hi) if lo < hi else (lo, lo)


def output_plan(path_file, pairs, sequences, args):
    """One walk over the path file for print_gap_filled_sequences (:533-598) and print_agp (:600-665), the two loops restated side by
    side -- they are not symmetric, see the comments.  pairs: (source, target) -> PairInfo with ``chosen_reversed``; sequences: name ->
    ScaffoldGaps; args: ``.min_gap`` (already one more than the option, as main() leaves it) and ``.soft_mask``.  -> OutputPlan:

    * records: per line with a tab, in order, (id, pieces) -- a piece is ("scaffold", name, lo, hi, flags), ("read", read id, lo, hi,
      flags) with lo <= hi and capi.NTL_STITCH_* flags, or ("N", count).  Scaffold slices are clamped to the scaffold; a read's are
      clamped by whoever knows its length (Python's slice would)
    * agp: the rows of the .agp file as tuples of its columns, the unassigned scaffolds' last
    * counters: the seven of print_filling_stats; printed: the scaffolds some path names; unassigned: the others, in order"""
    records, agp, printed = [], [], set()
    counters = dict.fromkeys(_COUNTERS, 0)
    overlap_gap = False  # outlives a line, as in the reference
    with open(path_file, "r") as fin:
        for line in fin:
            start, component_id = 1, 1
            line = line.strip().split("\t")
            if len(line) < 2:
                continue
            ctg_id, path = line
            path = path.split(" ")
            pieces = []
            for idx, node in enumerate(path):
                gap_match = _GAP.search(node)
                if gap_match:
                    gap_size = int(gap_match.group(1))
                    counters["num_gaps"] += 1
                    if gap_size == 1:  # tally_small_gaps (:697-704)
                        overlap_gap = True
                        counters["overlap_pts"] += 1
                    if args.min_gap >= gap_size > 1:
                        counters["small_gaps"] += 1
                    gap_size -= 1  # abyss-scaffold's gap is one more
                    pair = pairs.get((path[idx - 1], path[idx + 1]))
                    if pair is None:
                        pieces.append(("N", max(gap_size, 0)))
                        if gap_size > 0:  # the row is written, and neither it nor a skipped one advances component_id (`continue`, :625-627)
                            agp.append((ctg_id, start, start + gap_size - 1, component_id, "N", gap_size, "scaffold", "yes", "paired-ends"))
                            start += gap_size
                        continue
                    counters["potential_fills"] += 1
                    if pair.source_read_cut is None or pair.target_read_cut is None:
                        pieces.append(("N", max(pair.gap_size, 0)))  # the FASTA takes the pair's size, the AGP the path's (the same number)
                        agp.append((ctg_id, start, start + gap_size - 1, component_id, "N", gap_size, "scaffold", "yes", "paired-ends"))
                        start += gap_size
                    else:
                        counters["filled_gaps"] += 1
                        counters["old_anchor_used" if pair.old_anchor_used else "new_anchor_used"] += 1  # tally_anchors (:689-694)
                        if pair.chosen_reversed:
                            read_start, read_end, ori = pair.target_read_cut, pair.source_read_cut, "-"
                        else:
                            read_start, read_end, ori = pair.source_read_cut, pair.target_read_cut, "+"
                        flags = (capi.NTL_STITCH_REVCOMP if ori == "-" else 0) | (capi.NTL_STITCH_LOWER if args.soft_mask else 0)
                        pieces.append(("read", pair.chosen_read, read_start, max(read_start, read_end), flags))
                        if not read_end >= read_start + 1:
                            continue  # a fully eroded read: no row, component_id stays
                        agp.append((ctg_id, start, start + (read_end - read_start) - 1, component_id, "P", pair.chosen_read, read_start + 1,
                                    read_end, ori))
                        start += read_end - read_start
                else:
                    name = node.strip("+-")
                    printed.add(name)
                    scaf_start, scaf_end = sequences[name].get_cut_coordinates()
                    lo, hi = _slice(scaf_start, scaf_end, sequences[name].length)
                    flags = capi.NTL_STITCH_REVCOMP if node[-1] == "-" else 0
                    if overlap_gap:  # cleared even when the piece is empty
                        flags |= capi.NTL_STITCH_LOWER_FIRST
                        overlap_gap = False
                    pieces.append(("scaffold", name, lo, hi, flags))
                    if not scaf_end >= scaf_start + 1:
                        continue  # a fully eroded scaffold
                    agp.append((ctg_id, start, start + (scaf_end - scaf_start) - 1, component_id, "W", name, scaf_start + 1, scaf_end, node[-1]))
                    start += scaf_end - scaf_start
                component_id += 1
            records.append((ctg_id, pieces))
    unassigned = [name for name in sequences if name not in printed]
    for name in unassigned:  # the FASTA has the whole untrimmed sequence, the AGP the cut coordinates
        ctg_start, ctg_end = sequences[name].get_cut_coordinates()
        agp.append((name, ctg_start + 1, ctg_end, 1, "W", name, ctg_start + 1, ctg_end, "+"))
    return OutputPlan(records, agp, counters, printed, unassigned)


def print_filling_stats(counter, file=None):
    """print_filling_stats (:668-678)"""
    out = lambda *a, **kw: print(*a, file=file, **kw)
    out("\nGap filling summary:")
    out("Number of detected sequence joins", counter["num_gaps"], sep="\t")
    out("Number of overlap sequence joins", counter["overlap_pts"], sep="\t")
    out("Number of gaps smaller than threshold", counter["small_gaps"], sep="\t")
    out("Number of potentially fillable gaps", counter["potential_fills"], sep="\t")
    out("Number of filled gaps", counter["filled_gaps"], sep="\t")
    out("Number of pass 2 anchors used", counter["new_anchor_used"], sep="\t")
    out("Number of pass 1 anchors used", counter["old_anchor_used"], sep="\t")
    out()


def _record_segments(plan, sequences, scaffolds, reads):
    """per output record (header bytes, [(store, rec, lo, hi, flags)], bytes of text): stores 0 = scaffolds, 1 = reads, 2 = the headers
    of the call the record goes to (its `rec` is filled in there)"""
    fill = capi.NTL_STITCH_FILL
    for ctg_id, pieces in plan.records:
        segs, size = [], 0
        for piece in pieces:
            if piece[0] == "N":
                seg = (fill, ord("N"), 0, piece[1], 0)
            elif piece[0] == "scaffold":
                seg = (0, scaffolds.number[piece[1]], piece[2], piece[3], piece[4])
            else:
                rec = reads.number[piece[1]]
                lo, hi = _slice(piece[2], piece[3], int(reads.lengths[rec]))
                seg = (1, rec, lo, hi, piece[4])
            if seg[3] > seg[2]:
                segs.append(seg)
                size += seg[3] - seg[2]
        header = b">" + ctg_id.encode() + b"\n"
        yield header, segs, len(header) + size + 1
    for name in plan.unassigned:
        header = b">" + name.encode() + b"\n"
        rec = scaffolds.number[name]
        length = int(scaffolds.lengths[rec])
        yield header, [(0, rec, 0, length, 0)] if length else [], len(header) + length + 1


def _stitch_calls(records, max_bytes):
    """whole records per call, at most max_bytes of text each; a larger record goes alone"""
    call, size = [], 0
    for rec in records:
        if call and size + rec[2] > max_bytes:
            yield call
            call, size = [], 0
        call.append(rec)
        size += rec[2]
    if call:
        yield call


def print_gap_filled_sequences(pairs, sequences, scaffolds, reads, args, dev=None, max_bytes=STITCH_BYTES, plan=None, stats_file=None):
    """print_gap_filled_sequences (:533-598): writes ``args.o`` and prints the filling summary.  scaffolds, reads: Resident made with
    stitchable=True (their bytes are the sources); sequences: name -> ScaffoldGaps with the final cuts and trims.  Per call of
    Device.stitch whole output records of at most max_bytes of text together; the text comes back in pieces into page-locked memory and
    goes to the file through ntl_write_blob.  -> the OutputPlan."""
    dev = dev or anchor._default_device()
    if scaffolds.ascii is None or reads.ascii is None:
        raise ValueError("the scaffolds' and the reads' bytes must be resident (stitchable=True)")
    plan = plan or output_plan(args.path, pairs, sequences, args)
    write_stitched_records(dev, args.o, [scaffolds.ascii, reads.ascii], _record_segments(plan, sequences, scaffolds, reads), max_bytes)
    print_filling_stats(plan.counters, file=stats_file)
    return plan


def write_stitched_records(dev, path, stores, records, max_bytes=STITCH_BYTES, on_text=None):
    """Writes `path`: per record its header, its segments and a newline, assembled on the device (Device.stitch) from the resident
    `stores` (capi.Ascii).  records: (header bytes, [(store, rec, lo, hi, flags)], bytes of text) each; the headers of a call are
    one more store behind `stores`.  Whole records of at most max_bytes of text per call; the text comes back in pieces into
    page-locked memory and goes to the file through ntl_write_blob.  The writer of the gap filler's, the overlap stage's and the
    merge stage's FASTA.  path: a file name, or a file descriptor that is open for writing (it stays open).  on_text(text, call):
    called per stitch call with the capi.Stitched and the call's records while the text is on the device (the merge stage counts
    its called bases there)."""
    newline = (capi.NTL_STITCH_FILL, ord("\n"), 0, 1, 0)
    fd = path if isinstance(path, int) else os.open(path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o666)
    buf = None
    try:
        for call in _stitch_calls(records, max_bytes):
            segs = []
            for i, (header, rec_segs, _size) in enumerate(call):
                segs.append((len(stores), i, 0, len(header), 0))
                segs += rec_segs
                segs.append(newline)
            with dev.ascii([header for header, _segs, _size in call]) as headers, \
                    dev.stitch(list(stores) + [headers], np.array(segs, capi.STITCH_SEG_DT)) as text:
                total = text.nbytes
                if on_text is not None:
                    on_text(text, call)
                if buf is None or len(buf) < min(total, WRITE_PIECE):
                    dev.pinned_release(buf)
                    buf = dev.pinned_empty(min(total, WRITE_PIECE))
                for lo in range(0, total, len(buf)):
                    hi = min(total, lo + len(buf))
                    text.copy(lo, hi, buf)
                    if dev.L.ntl_write_blob(fd, buf.ctypes.data, hi - lo) != 0:
                        raise OSError(f"{path}: write failed")
    finally:
        if fd is not path:
            os.close(fd)
        dev.pinned_release(buf)


def print_agp(pairs, sequences, args, plan=None):
    """print_agp (:600-665): writes ``args.o + ".agp"``"""
    plan = plan or output_plan(args.path, pairs, sequences, args)
    with open(args.o + ".agp", "w") as out:
        for row in plan.agp:
            out.write("\t".join(str(col) for col in row) + "\n")
    return plan


def print_log_message(message):
    """:729-731"""
    print(datetime.datetime.today(), message, flush=True)


def print_parameters(args):
    """print_parameters (:733-758)"""
    print("Running ntLink gap-filling...\n")
    print("Parameters:")
    print("\t--path", args.path)
    print("\t--mappings", args.mappings)
    print("\t--trims", args.trims)
    print("\t-s", args.s)
    print("\t--reads", args.reads)
    print()
    print("\t-z", args.z)
    print("\t-k", args.k)
    print("\t-w", args.w)
    print("\t-t", args.t)
    print("\t--large_k", args.large_k)
    print("\t-x", args.x)
    print("\t--min_gap", args.min_gap)
    print("\t-o", args.o)
    if args.verbose:
        print("\t--verbose")
    if args.stringent:
        print("\t--stringent")
    if args.soft_mask:
        print("\t--soft_mask")
    print()


def patch_gaps(args, dev=None, max_bytes=STITCH_BYTES):
    """main() of the reference behind its argument parser (:786-836): the whole gap-filling stage.  args: the reference's namespace
    (path mappings trims s reads z k w t large_k x min_gap o stringent soft_mask sensitive verbose; it is not changed).  Writes
    ``args.o`` and ``args.o + ".agp"`` and prints the reference's log lines and the filling summary; the two masked temporary files
    of the reference are never written.  -> (pairs, sequences, OutputPlan)."""
    dev = dev or anchor._default_device()
    args = copy.copy(args)
    args.min_gap = args.min_gap + 1
    pairs = read_path_file_pairs(args.path, args.min_gap)
    print_log_message("Reading scaffolds..")
    with resident_scaffolds(args.s, dev=dev, stitchable=True) as scaffolds:
        sequences = {name: ScaffoldGaps(length=length) for name, length in zip(scaffolds.ids, scaffolds.lengths.tolist())}
        print_log_message("Reading trim coordinates..")
        read_trim_coordinates(sequences, args)
        print_log_message("Reading ntLink read mappings..")  # (read block by block while the reads are chosen)
        print_log_message("Choosing best read..")
        print_log_message("Finding masking points..")
        choose_gap_reads(pairs, args.mappings, sequences, args, dev=dev)
        print_log_message("Collecting reads...")
        with get_gap_fill_reads(args.reads, pairs, args, dev=dev, stitchable=True) as reads:
            print_log_message("Mapping long reads..")
            map_long_reads_resident(pairs, sequences, scaffolds, reads, args, dev=dev)
            print_log_message("Printing output scaffolds..")
            plan = output_plan(args.path, pairs, sequences, args)
            print_gap_filled_sequences(pairs, sequences, scaffolds, reads, args, dev=dev, max_bytes=max_bytes, plan=plan)
            print_log_message("Printing AGP file..")
            print_agp(pairs, sequences, args, plan=plan)
    print_log_message("DONE!")
    return pairs, sequences, plan
