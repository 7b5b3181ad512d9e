"""The merge stage: `MergeContigs -k2 FASTA PATH` of ABySS, the last step of `ntLink scaffold` (ntLink:253-259), which writes the scaffold
FASTA from the trimmed contigs and a path file.  ABySS is not part of the reference tree; the rules below were derived from the
reference's four shipped cases (tests/golden/ref/expected_outputs: `.trimmed_scafs.fa.gz` + `.trimmed_scafs.path` ->
`.stitch.abyss-scaffold.fa.gz`), whose six paths they reproduce byte for byte.  DESIGN.md says which rules rest on no fixture.

  path line   name<TAB>node node ...        a node is <contig>+, <contig>- or <n>N
  output      >name LEN 0 COMMENT\\nSEQ\\n   per path, in file order; SEQ on one line, LEN its length
    <contig>+   the contig's bytes as read, case kept          <contig>-   reverse complement (the stitch kernel's table), case kept
    <n>N        n - 1 bytes of N (abyss-scaffold's gap is one more, as overlap.py and gapfill.py account for)
    1N          no N at all; the first base of the next contig is lower-cased (NTL_STITCH_LOWER_FIRST)
    COMMENT     the nodes joined by `,`; with more than three, `first,...,last`
  Contigs that no path names come first, in input order, header line as read, sequence on one line.

The text is assembled on the device by ntl_stitch from the resident contigs (gapfill.write_stitched_records), and the called bases of
every output record are counted there too (ntl_stitched_base_counts, csrc/count_kernels.h): `fac_stats` makes the `abyss-fac` line of
them.  Nothing here computes on the host what the device is for: a missing library or GPU is an error."""
import collections
import mmap
import os
import re

import numpy as np

from . import capi

_GAP = re.compile(r"(\d+)N")
_NO_REC = -1  # Contigs.rec of a contig that is a lone N (an empty trim)


class Contigs:
    """What the merge needs of the contigs, in input order: ``ids``, per contig the record ``rec`` of the resident store its bytes
    are in and the slice [``lo``, ``hi``) of it (rec -1: a lone N, what the overlap stage writes where a trim leaves nothing), and
    the ``headers`` (the header line as read, without `>` and the newline; None: the id).  ``resident``: the gapfill.Resident the
    records are in, where the contigs are handed over resident (trimmed_contigs)."""

    def __init__(self, ids, rec, lo, hi, headers=None, resident=None):
        self.ids = list(ids)
        self.rec, self.lo, self.hi = (np.ascontiguousarray(a, np.int64) for a in (rec, lo, hi))
        self.headers = [rid.encode() for rid in self.ids] if headers is None else list(headers)
        self.resident = resident
        self.number = {rid: i for i, rid in enumerate(self.ids)}
        if len(self.number) != len(self.ids):
            raise ValueError("two contigs with the same id")
        if not len(self.ids) == len(self.rec) == len(self.lo) == len(self.hi) == len(self.headers):
            raise ValueError("ids, records, slices and headers must be of one length")

    @classmethod
    def whole(cls, ids, lengths, headers=None, resident=None):
        "every contig a whole record, in order"
        lengths = np.ascontiguousarray(lengths, np.int64)
        return cls(ids, np.arange(len(lengths)), np.zeros(len(lengths), np.int64), lengths, headers, resident)

    @classmethod
    def of(cls, records):
        "a Contigs as it is; a gapfill.Resident (.ids, .lengths) or [(id, length)]: whole records"
        if isinstance(records, cls):
            return records
        if hasattr(records, "ids") and hasattr(records, "lengths"):
            return cls.whole(records.ids, records.lengths, resident=records if getattr(records, "ascii", None) is not None else None)
        records = list(records)
        return cls.whole([rid for rid, _n in records], [n for _rid, n in records])


def trimmed_contigs(scaffolds, resident, k):
    """The contigs of `.trimmed_scafs.fa` without the file: trimmed coordinates mapped onto the UNTRIMMED resident records, by the
    writer's own rule (overlap._trimmed_records: omitted scaffolds left out, the header `id source_cut-target_cut`, a lone N where
    nothing is left).  scaffolds: id -> overlap.ScaffoldCut after the stage; resident: gapfill.resident_scaffolds(args.fasta,
    stitchable=True).  -> Contigs for merge_contigs(resident=...)."""
    from . import overlap
    ids, rec, lo, hi, headers = [], [], [], [], []
    for header, (seg,), _size in overlap._trimmed_records(scaffolds, resident, k):
        line = header[1:-1]
        headers.append(line)
        ids.append(line.split(None, 1)[0].decode())
        whole = seg[0] != capi.NTL_STITCH_FILL
        rec.append(seg[1] if whole else _NO_REC)
        lo.append(seg[2] if whole else 0)
        hi.append(seg[3] if whole else 1)
    return Contigs(ids, rec, lo, hi, headers, resident)


def fasta_headers(path):
    "the header lines of a FASTA file, in order, without `>` and the line end (a plain file is searched in place, not read line by line)"
    from . import seqio
    with open(path, "rb") as fh:
        plain = fh.read(2) != b"\x1f\x8b"
        if plain and os.fstat(fh.fileno()).st_size:
            with mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ) as mm:
                return [m.group(1) for m in re.finditer(rb"^>([^\r\n]*)", mm, re.M)]
    with seqio._open(path) as fh:
        return [line[1:].rstrip(b"\r\n") for line in fh if line[:1] == b">"]


class MergePlan(collections.namedtuple("MergePlan", "headers segs first seq_len n_unpathed")):
    """The output records of the merge, unpathed contigs first: ``headers`` (the header lines, `>` and newline included: the header
    store of the stitch), ``segs`` (capi.STITCH_SEG_DT, store 0 = the contigs; empty pieces dropped), ``first`` (record i is
    segs[first[i]:first[i + 1]]), ``seq_len`` (LEN of record i), ``n_unpathed``."""

    def records(self):
        "(header bytes, [(store, rec, lo, hi, flags)], bytes of text) per record: what gapfill.write_stitched_records takes"
        first = self.first.tolist()
        for i, header in enumerate(self.headers):
            yield header, self.segs[first[i]:first[i + 1]].tolist(), len(header) + int(self.seq_len[i]) + 1


def _segments(contigs, ci, minus, lower_first, gap):
    """per node its segment and its length: ci >= 0 the contig (minus, lower_first as 0 / 1), ci < 0 a gap of `gap` bytes"""
    n = len(ci)
    seg = np.zeros(n, capi.STITCH_SEG_DT)
    is_ctg = ci >= 0
    at = np.where(is_ctg, ci, 0)
    rec = np.where(is_ctg, contigs.rec[at] if len(contigs.rec) else 0, _NO_REC)
    lone = is_ctg & (rec == _NO_REC)
    copy = is_ctg & ~lone
    fill_byte = np.where(lone & (lower_first != 0), ord("n"), ord("N"))  # what LOWER_FIRST makes of a record that is one N
    seg["store"] = np.where(copy, 0, capi.NTL_STITCH_FILL)
    seg["rec"] = np.where(copy, rec, fill_byte)
    seg["lo"] = np.where(copy, contigs.lo[at] if len(contigs.lo) else 0, 0)
    seg["hi"] = np.where(copy, contigs.hi[at] if len(contigs.hi) else 0, np.where(lone, 1, gap))
    seg["flags"] = np.where(copy, capi.NTL_STITCH_REVCOMP * minus + capi.NTL_STITCH_LOWER_FIRST * lower_first, 0)
    return seg, seg["hi"].astype(np.int64) - seg["lo"].astype(np.int64)


def merge_plan(path_file, records):
    """The output of `MergeContigs -k2` as stitch segments.  records: Contigs, a gapfill.Resident or [(id, length)] (Contigs.of).
    -> MergePlan.  One loop over the nodes of the path file; lengths, offsets and segments are computed as arrays.  ValueError,
    naming the file, the line and the node, for: a contig that is not among the records; a contig used by two nodes; two contig
    nodes with no gap between them (the one-base overlap merge of -k2 cannot be derived from the fixtures) and two gaps in a row; a
    gap at either end of a path; `0N`; a node that does not end in +, - or N."""
    contigs = Contigs.of(records)
    names, comments, starts = [], [], [0]   # per path
    ci, minus, gap = [], [], []             # per node: the contig's number or -1, its sign, the gap's bytes
    used = {}
    with open(path_file, "r") as fin:
        for lineno, line in enumerate(fin, 1):
            fields = line.strip().split("\t")
            if len(fields) < 2:
                continue
            path = fields[1].split(" ")

            def refuse(node, why):
                return ValueError(f"{path_file}:{lineno}: node {node!r}: {why}")

            was_gap = None
            for at, node in enumerate(path):
                m = _GAP.fullmatch(node)
                if m:
                    if int(m.group(1)) == 0:
                        raise refuse(node, "a gap of 0N (abyss-scaffold's gap is one more than the bases it stands for)")
                    if at == 0 or at == len(path) - 1:
                        raise refuse(node, "a gap at the end of a path")
                    if was_gap:
                        raise refuse(node, "two gaps in a row")
                    ci.append(-1); minus.append(0); gap.append(int(m.group(1)) - 1)
                elif len(node) > 1 and node[-1] in "+-":
                    if was_gap is False:
                        raise refuse(node, "two contigs with no gap between them (the overlap merge of -k2 is not implemented)")
                    number = contigs.number.get(node[:-1])
                    if number is None:
                        raise refuse(node, f"no contig {node[:-1]} among the sequences")
                    if number in used:
                        raise refuse(node, f"contig {node[:-1]} is already used, at line {used[number]}")
                    used[number] = lineno
                    ci.append(number); minus.append(int(node[-1] == "-")); gap.append(0)
                else:
                    raise refuse(node, "a node must end in +, - or N")
                was_gap = bool(m)
            names.append(fields[0])
            comments.append(",".join(path) if len(path) <= 3 else f"{path[0]},...,{path[-1]}")
            starts.append(len(ci))
    ci, minus, gap = np.array(ci, np.int64), np.array(minus, np.int64), np.array(gap, np.int64)
    if len(gap) and int(gap.max()) >= 1 << 32:
        raise ValueError(f"{path_file}: a gap of 2^32 bases or more")
    behind_join = np.zeros(len(ci), np.int64)  # the contig behind a 1N gap: its first base is lower-cased
    behind_join[1:] = (ci[1:] >= 0) & (ci[:-1] < 0) & (gap[:-1] == 0)
    seg, length = _segments(contigs, ci, minus, behind_join, gap)
    starts = np.array(starts, np.int64)
    csum = np.concatenate([[0], np.cumsum(length)])
    path_len = csum[starts[1:]] - csum[starts[:-1]]
    kept = np.concatenate([[0], np.cumsum(length > 0)])
    # the contigs no path names, whole, in input order
    free = np.setdiff1d(np.arange(len(contigs.ids)), ci[ci >= 0], assume_unique=True) if len(contigs.ids) else np.zeros(0, np.int64)
    zeros = np.zeros(len(free), np.int64)
    fseg, flen = _segments(contigs, free.astype(np.int64), zeros, zeros, zeros)
    fkept = np.concatenate([[0], np.cumsum(flen > 0)])
    headers = [b">" + contigs.headers[i] + b"\n" for i in free.tolist()] + \
              [f">{name} {n} 0 {comment}\n".encode() for name, n, comment in zip(names, path_len.tolist(), comments)]
    first = np.concatenate([fkept, fkept[-1] + kept[starts[1:]]])
    return MergePlan(headers, np.concatenate([fseg[flen > 0], seg[length > 0]]), first.astype(np.int64),
                     np.concatenate([flen, path_len]).astype(np.int64), len(free))


def record_offsets(call):
    """The pieces of one stitch call's text as ascending offsets, for Stitched.base_counts: [0, end of header 0, end of sequence 0,
    end of header 1, ...] and the text's end -- piece 2i + 1 is the sequence of record i, the others are header lines and newlines.
    call: [(header, segments, bytes of text)]."""
    sizes = np.fromiter((size for _h, _s, size in call), np.int64, len(call))
    heads = np.fromiter((len(h) for h, _s, _size in call), np.int64, len(call))
    begin = np.concatenate([[0], np.cumsum(sizes)])
    off = np.empty(2 * len(call) + 2, np.uint64)
    off[0] = 0
    off[1:-1:2] = begin[:-1] + heads
    off[2:-1:2] = begin[1:] - 1
    off[-1] = begin[-1]
    return off


MergeResult = collections.namedtuple("MergeResult", "plan counts")


def merge_contigs(fasta, path_file, out, dev=None, resident=None, max_bytes=None):
    """`MergeContigs -k2 fasta path_file > out`: writes the scaffold FASTA (out: a file name, or an open file descriptor) and counts
    the called bases of every record it wrote.  The contigs come from gapfill.resident_scaffolds(fasta, stitchable=True), or, with
    resident= (trimmed_contigs: the overlap stage's store, `fasta` is then not read), from the records already on the device; the
    bytes written are the same either way.  Whole records of at most max_bytes of text per stitch call (a larger one goes alone).
    -> MergeResult(plan, counts): counts[i], u64, the bytes of record i's sequence that are one of ACGTacgt (for fac_stats)."""
    from . import anchor, gapfill
    dev = dev or anchor._default_device()
    own = resident is None
    if own:
        store = gapfill.resident_scaffolds(fasta, dev=dev, stitchable=True)
    else:
        store = resident.resident
        if store is None or store.ascii is None:
            raise ValueError("resident= needs the contigs' bytes on the device (trimmed_contigs over a stitchable Resident)")
    try:
        if own:
            headers = fasta_headers(fasta)
            if [h.split(None, 1)[0].decode() if h.split(None, 1) else "" for h in headers] != store.ids:
                raise ValueError(f"{fasta}: the header lines do not match the records that were read")
            contigs = Contigs.whole(store.ids, store.lengths, headers, store)
        else:
            contigs = resident
        plan = merge_plan(path_file, contigs)
        counts = []

        def count(text, call):
            counts.append(text.base_counts(record_offsets(call))[1::2])

        gapfill.write_stitched_records(dev, out, [store.ascii], plan.records(), max_bytes or gapfill.STITCH_BYTES, on_text=count)
    finally:
        if own:
            store.close()
    return MergeResult(plan, np.concatenate(counts) if counts else np.zeros(0, np.uint64))


def merge_after_overlap(args, out, dev=None, max_bytes=None):
    """overlap.overlap_sequences(args) and then the merge of what it wrote, from the store the overlap stage still holds: the
    `.trimmed_scafs.fa` it just wrote is not read back (the path file, a few lines, is).  The bytes of `out` are those of
    merge_contigs(args.p + ".trimmed_scafs.fa", args.p + ".trimmed_scafs.path", out).  -> (scaffolds, new paths, MergeResult)."""
    from . import overlap
    got = []

    def merge(scaffolds, resident):
        got.append(merge_contigs(None, args.p + ".trimmed_scafs.path", out, dev, resident=trimmed_contigs(scaffolds, resident, args.k),
                                 max_bytes=max_bytes))

    scaffolds, new_paths = overlap.overlap_sequences(args, dev, with_resident=merge)
    return scaffolds, new_paths, got[0]


FAC_COLUMNS = ("n", "n:500", "L50", "min", "N75", "N50", "N25", "E-size", "max", "sum")


def fac_stats(counts, min_len=500):
    """The numbers of `abyss-fac -t min_len` from the called bases of every record -> dict over FAC_COLUMNS (the second key is
    `n:<min_len>`).  n counts every record, the rest the records of at least min_len called bases: Nxx is the smallest size whose
    records and all smaller ones hold at least ceil((1 - xx/100) * sum) bases, L50 the number of records of at least N50, E-size
    sum(size^2) / sum truncated.  No record of that size: zeros."""
    counts = np.ascontiguousarray(counts, np.uint64).astype(object)  # Python integers: squares of 10^9 and their sums stay exact
    sizes = sorted(int(c) for c in counts if c >= min_len)
    keys = tuple(f"n:{min_len}" if key == "n:500" else key for key in FAC_COLUMNS)
    if not sizes:
        return dict(zip(keys, (len(counts),) + (0,) * 9))
    total = sum(sizes)

    def weighted(num, den):
        "the smallest size with at least ceil(total * num / den) bases in the records up to it"
        want, seen = -(-total * num // den), 0
        for size in sizes:
            seen += size
            if seen >= want:
                return size
        return sizes[-1]

    n50 = weighted(1, 2)
    return dict(zip(keys, (len(counts), len(sizes), sum(1 for s in sizes if s >= n50), sizes[0], weighted(1, 4), n50, weighted(3, 4),
                           sum(s * s for s in sizes) // total, sizes[-1], total)))


def fac_text(stats, name):
    "the two lines `abyss-fac` prints: the column names and the numbers, tab-separated, `name` last"
    return "\t".join(list(stats) + ["name"]) + "\n" + "\t".join(str(v) for v in stats.values()) + f"\t{name}\n"
