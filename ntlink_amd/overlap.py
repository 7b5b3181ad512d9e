"""Consumer of the overlap-stage sketch: the minimizers `ntlink_overlap_sequences.py` keeps per contig.

`indexlr --long --pos -k 15 -w 5` (one minimizer per ~3 bases, ntLink:243-251) feeds `read_minimizers` /
`read_minimizers_path` / `read_minimizer_line` of bin/ntlink_overlap_sequences.py:145-190: minimizers outside the contig's valid
regions are dropped, and so is every hash that occurs more than once on the contig.  Here the text is parsed by the native
TSV reader (csrc/ntl_io.cpp, `H:pos` tokens) and the filter runs on the GPU (csrc/overlap_kernels.h, `ntl_overlap_filter`);
`filter_sketch` is the same on a device-resident sketch, without any text in between.  The functions of the reference keep
their names, arguments and return shapes.

The stage behind the filter is here too (`overlap_sequences`, the reference's main()): `merge_overlapping_pathfile` decides the cut
points of every adjacent, overlapping pair of a path file in one device pass (csrc/overlap_cut_kernels.h, `ntl_overlap_cuts` -- the
reference's merge_overlapping :341-417 builds an igraph graph per pair) and applies them on the host in file order through
`ScaffoldCut`, and the four writers give `<prefix>.trimmed_scafs.{path,tsv,agp,fa}`; the FASTA is assembled on the device from the
resident bytes (gapfill.write_stitched_records).  Without a minimizer file the contigs with a valid region are sketched here, whole,
at (k, 5): no ntlink_filter_sequences.py, no indexlr and no text in between."""
import io
import os
import re
import tempfile
from collections import defaultdict

import numpy as np

from . import capi, formats

final_sequence_marker_re = re.compile(r"^LAST(ntLink_\d+)$")  # bin/ntlink_overlap_sequences.py:21


def is_in_valid_region(pos, valid_minimizer_positions):
    "True if the minimizer is in a valid position for overlap detection (bin/ntlink_overlap_sequences.py:138-143)"
    return any(start <= pos <= end for start, end in valid_minimizer_positions)


def _regions(names, valid_mx_positions):
    """CSR arrays of the valid regions of the named sequences (none for names outside valid_mx_positions); regions that
    cannot contain a position (end < 0 or end < start) are left out, negative starts clamp to 0"""
    off = np.zeros(len(names) + 1, np.uint64)
    starts, ends = [], []
    for i, name in enumerate(names):
        for start, end in valid_mx_positions.get(name, ()):
            if end < 0 or end < start:
                continue
            starts.append(max(0, min(int(start), 0xFFFFFFFF)))
            ends.append(min(int(end), 0xFFFFFFFF))
        off[i + 1] = len(starts)
    return off, np.array(starts, np.uint32), np.array(ends, np.uint32)


def filter_sketch(dev, sketch, names, valid_mx_positions):
    """Device-resident sketch (e.g. dev.sketch(batch, 15, 5)) -> (mx_off u64[n+1], hash u64, pos u32) of the kept
    minimizers, sequences in input order."""
    off, rs, re_ = _regions(names, valid_mx_positions)
    with dev.overlap_filter(sketch, off, rs, re_) as kept:
        mx_off, h, p, _ = kept.download()
    return mx_off, h, p


def _to_dicts(names, in_off, mx_off, h, p, valid_mx_positions, mx_info, mxs):
    for i, name in enumerate(names):
        if name not in valid_mx_positions or in_off[i + 1] == in_off[i]:
            continue  # a line without a minimizer column is skipped before anything is stored (:173-174)
        a, b = int(mx_off[i]), int(mx_off[i + 1])
        keys = [str(x) for x in h[a:b].tolist()]
        mx_info[name] = {k: (name, q) for k, q in zip(keys, p[a:b].tolist())}
        mxs[name] = [keys]


def _read_blocks(dev, path, valid_mx_positions, mx_info, mxs):
    seen = set()
    for names, _lens, mx_off, h, p, s in formats.read_indexlr(path, False, max_bytes=256 << 20, with_strand=False):
        names = list(names)
        for n in names:
            if n in valid_mx_positions:
                if n in seen:
                    # the reference would carry the first line's dict into the second one (bin/ntlink_overlap_sequences.py:181);
                    # indexlr never prints an id twice, so this is an input error here
                    raise ValueError(f"sequence id {n} occurs on more than one line of the minimizer file")
                seen.add(n)
        with dev.sketch_from_arrays(mx_off, h, p, s) as sk:
            k_off, kh, kp = filter_sketch(dev, sk, names, valid_mx_positions)
        _to_dicts(names, mx_off, k_off, kh, kp, valid_mx_positions, mx_info, mxs)


def read_minimizers(tsv_filename, valid_mx_positions, dev=None):
    """Read the minimizers from a file, removing duplicate minimizers for a given contig
    (bin/ntlink_overlap_sequences.py:145-155) -> (mx_info: contig -> mx -> (contig, position), mxs: contig -> [[mx, ...]])"""
    own = dev is None
    if own:
        from . import capi
        dev = capi.Device(0)
    try:
        mx_info, mxs = defaultdict(dict), {}
        _read_blocks(dev, tsv_filename, valid_mx_positions, mx_info, mxs)
        return mx_info, mxs
    finally:
        if own:
            dev.close()


def read_minimizers_path(mx_reader, valid_mx_positions, dev=None):
    """Read in the minimizers for the given path, stopping at the LAST marker (bin/ntlink_overlap_sequences.py:157-168):
    consumes lines of the open text stream up to and including the `LASTntLink_<n>` line."""
    lines = []
    for line in mx_reader:
        name = line.strip().split("\t")[0]
        if re.search(final_sequence_marker_re, name):
            break
        lines.append(line if line.endswith("\n") else line + "\n")
    mx_info, mxs = defaultdict(dict), {}
    if not lines:
        return mx_info, mxs
    own = dev is None
    if own:
        from . import capi
        dev = capi.Device(0)
    try:
        with tempfile.NamedTemporaryFile("w", suffix=".tsv", dir=os.environ.get("TMPDIR")) as tmp:
            tmp.writelines(lines)
            tmp.flush()
            _read_blocks(dev, tmp.name, valid_mx_positions, mx_info, mxs)
        return mx_info, mxs
    finally:
        if own:
            dev.close()


# ---------------------------------------------------------------- the stage behind the filter (bin/ntlink_overlap_sequences.py:24-127, 324-333, 419-608)

OVERLAP_W = 5                 # ntLink:76, small_w
BATCH_BASES = 1 << 30         # bases of contigs sketched per device pass of the fused form
GAP_RE = re.compile(r"^(\d+)N$")  # main(), :590


class ScaffoldCut:
    """A scaffold and its two cut points (bin/ntlink_overlap_sequences.py:24-127).  The first orientation it is given fixes the
    defaults -- '+': target cut 0, source cut length; '-': the other way round -- a second, different one is an AssertionError, and so
    is a cut that was set before.  The stage itself gives `length=` in place of a sequence: its writers read the resident bytes."""

    def __init__(self, ctg_id, sequence=None, store_seq=False, length=None):
        self.ctg_id = ctg_id
        self.length = len(sequence) if length is None else int(length)
        self.sequence = sequence if store_seq else None
        self._ori = self._source_cut = self._target_cut = None
        self._source_cut_flag = self._target_cut_flag = self._omit_flag = False

    @property
    def ori(self):
        return self._ori

    @ori.setter
    def ori(self, orientation):
        if self._ori is not None and self._ori != orientation:
            raise AssertionError("Ori is already set")
        if orientation not in ("+", "-"):
            raise ValueError("Orientation must be + or -")
        if self._ori is None:
            self._target_cut, self._source_cut = (0, self.length) if orientation == "+" else (self.length, 0)
        self._ori = orientation

    def _unset(self, cut, plus_default, minus_default):
        return not ((self._ori == "+" and cut != plus_default) or (self._ori == "-" and cut != minus_default))

    @property
    def source_cut(self):
        return self._source_cut

    @source_cut.setter
    def source_cut(self, pos):
        if not self._unset(self._source_cut, self.length, 0):
            raise AssertionError("Source cut is already set")
        self._source_cut, self._source_cut_flag = pos, True

    @property
    def target_cut(self):
        return self._target_cut

    @target_cut.setter
    def target_cut(self, pos):
        if not self._unset(self._target_cut, 0, self.length):
            raise AssertionError("Target cut is already set")
        self._target_cut, self._target_cut_flag = pos, True

    def omit_sequence(self):
        "the trims crossed: the sequence stays out of every output"
        self._omit_flag = True

    def is_omitted_sequence(self):
        return self._omit_flag

    def adjust_source_cut(self, k):
        "the source cut, k further on for a '-' node whose cut was set: the minimizer's position is its k-mer's start"
        return self._source_cut + k if self._ori == "-" and self._source_cut_flag else self._source_cut

    def adjust_target_cut(self, k):
        return self._target_cut + k if self._ori == "-" and self._target_cut_flag else self._target_cut

    def get_trim_coordinates(self, k):
        "(start, end) of what is kept of the scaffold, on its forward strand"
        if self._ori == "+":
            return self._target_cut, self._source_cut
        if self._ori == "-":
            return self.adjust_source_cut(k), self.adjust_target_cut(k)
        if self._ori is None:
            return 0, self.length
        raise ValueError("Orientation should be +, - or None")

    def check_valid_trims(self, k):
        start, end = self.get_trim_coordinates(k)
        return True if self._ori is None else start < end

    def __str__(self):
        return f"{self.ctg_id}{self._ori} {self.length} - s:{self._source_cut} t:{self._target_cut}"


class ScaffoldGraph:
    """What the stage reads of the scaffold graph: the estimated distance `d` of every edge (the reference keeps an igraph graph)."""

    def __init__(self):
        self.vertices, self.d, self.n = set(), {}, {}

    def has_edge(self, source, target):
        return (source, target) in self.d


_DOT_SCAF_NUM = re.compile(r"graph \[scaf_num=(\S+)\]")
_DOT_NODE = re.compile(r'"(\S+[+-])"\s+\[l=\d+\]')
_DOT_EDGE = re.compile(r'"(\S+[+-])"\s+->\s+"(\S+[+-])"\s+\[d=(-?\d+)\s+e=\d+\s+n=(\d+)\]')


def read_scaffold_graph(in_graph_file):
    """The scaffold graph in dot format (bin/ntlink_utils.py:90-144) -> (ScaffoldGraph, scaf_num): the first line is the header, then
    nodes `"name+" [l=..]`, edges `"a+" -> "b-" [d=.. e=.. n=..]`, `graph [scaf_num=..]` and the closing brace.  Any other line is
    an error (the reference prints and exits)."""
    graph, scaf_num = ScaffoldGraph(), None
    with open(in_graph_file) as fh:
        for number, line in enumerate(fh):
            line = line.strip()
            if number == 0:
                continue
            node = _DOT_NODE.search(line)
            if node:
                graph.vertices.add(node.group(1))
                continue
            edge = _DOT_EDGE.search(line)
            if edge:
                graph.d[edge.group(1), edge.group(2)] = int(edge.group(3))
                graph.n[edge.group(1), edge.group(2)] = int(edge.group(4))
                continue
            num = _DOT_SCAF_NUM.search(line)
            if num:
                try:
                    scaf_num = int(num.group(1))
                except ValueError:
                    scaf_num = None
            elif line != "}":
                raise ValueError(f"{in_graph_file}: unexpected line in the dot file: {line}")
    return graph, scaf_num


def has_estimated_overlap(graph, source, target):
    "True if the graph has the edge and its distance estimate is negative (bin/ntlink_utils.py:56-63)"
    return graph.has_edge(source, target) and graph.d[source, target] < 0


def _flip(node):
    return node[:-1] + ("-" if node[-1] == "+" else "+")


def normalize_path(path_sequence, gap_re):
    """The path as it is or reversed with every sign flipped, so that its first contig's name is the smaller (bin/ntlink_utils.py:177-187)"""
    if path_sequence[0].strip("+-") < path_sequence[-1].strip("+-"):
        return path_sequence
    return [node if re.search(gap_re, node) else _flip(node) for node in reversed(path_sequence)]


def find_valid_mx_region(scaf_noori, scaf_ori, scaffolds, overlap, args, source=True):
    "(start, end) of the scaffold end that may hold the overlap of estimated size -overlap (bin/ntlink_utils.py:189-197)"
    length, size = scaffolds[scaf_noori].length, overlap * -1
    if (scaf_ori == "+") == bool(source):
        return (length - size - args.k) - int(size * args.f), length
    return 0, int(size * (args.f + 1))


def _path_lines(path_file, gap_re):
    with open(path_file) as fh:
        for line in fh:
            path_id, path_seq = line.strip().split("\t")
            yield path_id, normalize_path(path_seq.split(" "), gap_re)


def _overlap_triples(path_seq, gap_re, graph, args):
    "(index of the source in path_seq, estimated distance) of every triple the stage looks at (:461-468)"
    for i, gap in enumerate(path_seq[1:-1]):
        gap_match = re.search(gap_re, gap)
        if gap_match and int(gap_match.group(1)) <= args.g + 1 and has_estimated_overlap(graph, path_seq[i], path_seq[i + 2]):
            yield i, graph.d[path_seq[i], path_seq[i + 2]]


def find_valid_mx_regions(args, gap_re, graph, scaffolds):
    "scaffold -> [(start, end)]: where minimizers count for overlap detection (bin/ntlink_utils.py:146-175)"
    valid_regions = {}
    for _path_id, path_seq in _path_lines(args.path, gap_re):
        for i, d in _overlap_triples(path_seq, gap_re, graph, args):
            source, target = path_seq[i], path_seq[i + 2]
            for name in (source.strip("+-"), target.strip("+-")):
                if name not in scaffolds:
                    raise ValueError(f"pair {source} {target}: contig {name} is not in the FASTA file")
            valid_regions.setdefault(source.strip("+-"), []).append(find_valid_mx_region(source.strip("+-"), source[-1], scaffolds, d, args))
            valid_regions.setdefault(target.strip("+-"), []).append(find_valid_mx_region(target.strip("+-"), target[-1], scaffolds, d, args, source=False))
    return valid_regions


def set_scaffold_info(ctg_ori, pos, scaffolds, cut_type):
    "orientation and one cut of a scaffold (:324-333)"
    ctg, orientation = ctg_ori.strip("+-"), ctg_ori[-1]
    scaffolds[ctg].ori = orientation
    if cut_type == "source":
        scaffolds[ctg].source_cut = pos
    elif cut_type == "target":
        scaffolds[ctg].target_cut = pos
    else:
        raise ValueError("cut_type must be set to source or target")


def check_valid_overlap_trims(path, scaffolds, args):
    """A node whose two trims cross is taken out of the path with the gap behind it, the gap in front of it becomes `g + 1`, and the
    scaffold is omitted from every output (:419-444)."""
    gap_re, out, skip_gap = re.compile(r"(\d)N"), [], False
    for node in path:
        if re.search(gap_re, node):
            if not skip_gap:
                out.append(node)
            skip_gap = False
            continue
        scaffold = scaffolds[node.strip("+-")]
        if scaffold.source_cut is not None and scaffold.target_cut is not None and not scaffold.check_valid_trims(args.k):
            assert re.search(gap_re, out[-1])
            out[-1] = f"{args.g + 1}N"
            skip_gap = True
            scaffold.omit_sequence()
        else:
            out.append(node)
    return out


class _Pairs:
    """The qualifying pairs of a path file in file order: per pair its path line, nodes, names and the record ntl_overlap_cuts takes
    (sequence numbers filled in per device pass)."""

    def __init__(self, args, gap_re, graph, scaffolds):
        self.lines, self.pairs = [], []
        for path_id, path_seq in _path_lines(args.path, gap_re):
            first = len(self.pairs)
            for i, d in _overlap_triples(path_seq, gap_re, graph, args):
                self.pairs.append(self._pair(path_seq[i], path_seq[i + 2], d, scaffolds, args, len(self.lines), i))
            self.lines.append((path_id, path_seq, first, len(self.pairs)))

    @staticmethod
    def _pair(source, target, d, scaffolds, args, line, at):
        names = source.strip("+-"), target.strip("+-")
        what = f"{source} {target}"
        if names[0] == names[1]:
            raise ValueError(f"pair {what}: source and target are the same contig")
        for name in names:
            if name not in scaffolds:
                raise ValueError(f"pair {what}: contig {name} is not in the FASTA file")
        regions = find_valid_mx_region(names[0], source[-1], scaffolds, d, args), find_valid_mx_region(names[1], target[-1], scaffolds, d, args, source=False)
        rec = []
        for (start, end), name in zip(regions, names):
            start = max(0, start)
            if end < start or max(end, scaffolds[name].length) > 0xFFFFFFFF:
                raise ValueError(f"pair {what}: the valid region {start}..{end} of {name} (length {scaffolds[name].length}) does not fit 32 bits")
            rec += [start, end]
        signs = (capi.NTL_OVERLAP_SRC_MINUS if source[-1] == "-" else 0) | (capi.NTL_OVERLAP_TGT_MINUS if target[-1] == "-" else 0)
        return {"line": line, "at": at, "names": names, "what": what,
                "rec": (0, 0, *rec, scaffolds[names[0]].length, scaffolds[names[1]].length, signs, 0)}

    def records(self, lo, hi, number):
        "pairs lo..hi as OVERLAP_PAIR_DT, their contigs numbered by `number`"
        out = np.zeros(hi - lo, capi.OVERLAP_PAIR_DT)
        for i, pair in enumerate(self.pairs[lo:hi]):
            for name in pair["names"]:
                if name not in number:
                    raise ValueError(f"pair {pair['what']}: contig {name} has no line in the minimizer file")
            out[i] = (number[pair["names"][0]], number[pair["names"][1]]) + pair["rec"][2:]
        return out


def _cuts_fused(dev, pairs, resident, valid_mx_positions, k, batch_bases):
    """The fused form: per batch of whole path lines the contigs with a valid region -- copied unmasked from the resident batch, so
    that every window is the whole contig's -- sketched at (k, 5), filtered and cut, all on the resident records."""
    out = np.zeros(len(pairs.pairs), capi.OVERLAP_CUT_DT)
    lengths = resident.lengths
    at = 0
    while at < len(pairs.lines):
        names, number, bases, end = [], {}, 0, at
        while end < len(pairs.lines) and (end == at or bases < batch_bases):
            for pair in pairs.pairs[pairs.lines[end][2]:pairs.lines[end][3]]:
                for name in pair["names"]:
                    if name not in number:
                        number[name] = len(names)
                        names.append(name)
                        bases += int(lengths[resident.number[name]])
            end += 1
        lo, hi = pairs.lines[at][2], pairs.lines[end - 1][3]
        at = end
        if hi == lo:
            continue
        recs = np.array([resident.number[name] for name in names], np.uint32)
        off, rs, re_ = _regions(names, valid_mx_positions)
        with dev.batch_mask(resident.batch, recs, np.zeros(len(recs), np.uint32), lengths[recs]) as whole, \
                dev.sketch(whole, k, OVERLAP_W) as sk, dev.overlap_filter(sk, off, rs, re_) as kept:
            out[lo:hi] = dev.overlap_cuts(kept, pairs.records(lo, hi, number))
    return out


def _cuts_tsv(dev, pairs, tsv_filename, valid_mx_positions):
    """The TSV form: the file goes through the native reader and the filter block by block (`LASTntLink_n` marker lines are names
    without regions: they keep nothing); the kept minimizers of all blocks -- contig ends only -- are one sketch for ntl_overlap_cuts.
    A contig that ntlink_filter_sequences.py printed for two paths keeps its first line."""
    number, offs, hs, ps = {}, [0], [], []
    for names, _lens, mx_off, h, p, s in formats.read_indexlr(tsv_filename, False, max_bytes=256 << 20, with_strand=False):
        names = list(names)
        with dev.sketch_from_arrays(mx_off, h, p, s) as sk:
            k_off, kh, kp = filter_sketch(dev, sk, names, valid_mx_positions)
        for i, name in enumerate(names):
            if name not in valid_mx_positions or name in number or mx_off[i + 1] == mx_off[i]:
                continue
            number[name] = len(number)
            hs.append(kh[int(k_off[i]):int(k_off[i + 1])])
            ps.append(kp[int(k_off[i]):int(k_off[i + 1])])
            offs.append(offs[-1] + len(hs[-1]))
    out = np.zeros(len(pairs.pairs), capi.OVERLAP_CUT_DT)
    if not pairs.pairs:
        return out
    recs = pairs.records(0, len(pairs.pairs), number)
    h = np.concatenate(hs) if hs else np.zeros(0, np.uint64)
    p = np.concatenate(ps) if ps else np.zeros(0, np.uint32)
    with dev.sketch_from_arrays(np.array(offs, np.uint64), h, p, np.ones(len(h), np.uint8)) as kept:
        out[:] = dev.overlap_cuts(kept, recs)
    return out


def overlap_cuts(args, gap_re, graph, scaffolds, valid_mx_positions, dev, resident=None, batch_bases=BATCH_BASES):
    """One device pass over every qualifying pair of args.path -> (_Pairs, OVERLAP_CUT_DT records in file order).  args.m: the
    minimizer TSV, "-" for standard input, None for the fused form (which needs `resident`, gapfill.resident_scaffolds of args.fasta)."""
    pairs = _Pairs(args, gap_re, graph, scaffolds)
    if getattr(args, "m", None) is None:
        if resident is None:
            raise ValueError("the fused form sketches the resident scaffolds: resident= is needed when args.m is None")
        return pairs, _cuts_fused(dev, pairs, resident, valid_mx_positions, args.k, batch_bases)
    return pairs, _cuts_tsv(dev, pairs, "/dev/stdin" if args.m == "-" else args.m, valid_mx_positions)


def merge_overlapping_pathfile(args, gap_re, graph, scaffolds, valid_mx_positions, dev=None, resident=None, batch_bases=BATCH_BASES):
    """Goes through the path file, trims the overlapping pairs and writes `args.p + ".trimmed_scafs.path"` (:447-479) -> path id ->
    new path.  The cut points of all pairs come from one device pass (overlap_cuts); the paths are then walked in file order, every
    found cut applied through set_scaffold_info -- the assertions of ScaffoldCut fire where the reference's would -- its gap rewritten
    to `{args.outgap}N`, and check_valid_overlap_trims applied per path.  The file is written once every path is done."""
    from . import anchor
    dev = dev or anchor._default_device()
    pairs, cuts = overlap_cuts(args, gap_re, graph, scaffolds, valid_mx_positions, dev, resident, batch_bases)
    my_paths = {}
    for path_id, path_seq, first, last in pairs.lines:
        found = {pairs.pairs[i]["at"]: cuts[i] for i in range(first, last)}
        new_path = []
        for at, (source, gap, target) in enumerate(zip(path_seq, path_seq[1:], path_seq[2:])):
            if not re.search(gap_re, gap):
                continue
            cut = found.get(at)
            if cut is not None and cut["status"] & capi.NTL_OVERLAP_CUT:
                set_scaffold_info(source, int(cut["src_cut"]), scaffolds, "source")
                set_scaffold_info(target, int(cut["tgt_cut"]), scaffolds, "target")
                gap = f"{args.outgap}N"
            if not new_path:
                new_path.append(source)
            new_path += [gap, target]
        my_paths[path_id] = check_valid_overlap_trims(new_path, scaffolds, args)
    with open(args.p + ".trimmed_scafs.path", "w") as out:
        for path_id, _seq, _first, _last in pairs.lines:
            out.write(f"{path_id}\t{' '.join(my_paths[path_id])}\n")
    return my_paths


def print_trim_coordinates(args, scaffolds):
    "`args.p + \".trimmed_scafs.tsv\"`: name, start and end of what is kept of every scaffold that is not omitted (:503-512)"
    with open(args.p + ".trimmed_scafs.tsv", "w") as out:
        for scaffold in scaffolds.values():
            if not scaffold.is_omitted_sequence():
                start, end = scaffold.get_trim_coordinates(args.k)
                out.write(f"{scaffold.ctg_id}\t{start}\t{end}\n")


def print_agp_file(paths, scaffolds, args):
    """`args.p + ".trimmed_scafs.agp"` (:514-548): per path its trimmed contigs and its gaps -- a gap of `nN` is n - 1 bases, and a
    1N gap gives no row and takes no component number -- then every scaffold no path printed, omitted ones left out."""
    gap_re, printed = re.compile(r"(\d+)N"), set()
    with open(args.p + ".trimmed_scafs.agp", "w") as out:
        for path_id, path in paths.items():
            start, component = 1, 1
            for node in path:
                gap_match = re.search(gap_re, node)
                if gap_match:
                    size = int(gap_match.group(1)) - 1
                    if size == 0:
                        continue
                    out.write(f"{path_id}\t{start}\t{start + size - 1}\t{component}\tN\t{size}\tscaffold\tyes\tpaired-ends\n")
                    start += size
                else:
                    contig, ori = node.strip("+-"), node[-1]
                    lo, hi = scaffolds[contig].get_trim_coordinates(args.k)
                    out.write(f"{path_id}\t{start}\t{start + (hi - lo) - 1}\t{component}\tW\t{contig}\t{lo + 1}\t{hi}\t{ori}\n")
                    start += hi - lo
                    printed.add(contig)
                component += 1
        for name, scaffold in scaffolds.items():
            if name not in printed and not scaffold.is_omitted_sequence():
                lo, hi = scaffold.get_trim_coordinates(args.k)
                out.write(f"{scaffold.ctg_id}\t1\t{hi - lo}\t1\tW\t{scaffold.ctg_id}\t{lo + 1}\t{hi}\t+\n")


def _trimmed_records(scaffolds, resident, k):
    "per record of the FASTA file that is not omitted: header, its one segment (a lone N for an empty slice), bytes of text"
    from . import gapfill
    for rec, name in enumerate(resident.ids):
        scaffold = scaffolds[name]
        if scaffold.is_omitted_sequence():
            continue
        length = int(resident.lengths[rec])
        lo, hi = (0, length) if scaffold.ori is None else gapfill._slice(*scaffold.get_trim_coordinates(k), length)
        header = f">{scaffold.ctg_id} {scaffold.source_cut}-{scaffold.target_cut}\n".encode()
        seg = (0, rec, lo, hi, 0) if hi > lo else (capi.NTL_STITCH_FILL, ord("N"), 0, 1, 0)
        yield header, [seg], len(header) + max(hi - lo, 1) + 1


def print_trimmed_scaffolds(args, scaffolds, resident=None, dev=None, max_bytes=None):
    """`args.p + ".trimmed_scafs.fa"` (:481-501): every record of args.fasta that is not omitted, cut to its trim coordinates, with
    the header `>name source_cut-target_cut` (`None-None` for a scaffold no pair touched) and a lone N where nothing is left.
    resident: gapfill.resident_scaffolds(args.fasta, stitchable=True); the text is assembled on the device from its bytes."""
    from . import anchor, gapfill
    dev = dev or anchor._default_device()
    own = resident is None
    if own:
        resident = gapfill.resident_scaffolds(args.fasta, dev=dev, stitchable=True)
    try:
        if resident.ascii is None:
            raise ValueError("the scaffolds' bytes must be resident (stitchable=True)")
        gapfill.write_stitched_records(dev, args.p + ".trimmed_scafs.fa", [resident.ascii], _trimmed_records(scaffolds, resident, args.k),
                                       max_bytes or gapfill.STITCH_BYTES)
    finally:
        if own:
            resident.close()


def read_fasta_file_trim_prep(resident):
    "scaffold id -> ScaffoldCut, in the order of the FASTA file (:193-202), from the resident scaffolds' ids and lengths"
    return {name: ScaffoldCut(name, length=length) for name, length in zip(resident.ids, resident.lengths.tolist())}


OUTPUT_SUFFIXES = (".trimmed_scafs.path", ".trimmed_scafs.tsv", ".trimmed_scafs.agp", ".trimmed_scafs.fa")


def overlap_sequences(args, dev=None, batch_bases=BATCH_BASES, with_resident=None):
    """main() of the reference behind its argument parser (:583-608): the whole overlap stage.  args: the reference's namespace (m f
    path fasta k d g outgap p v trim_info; it is not changed), m=None for the fused form.  Writes `args.p + ".trimmed_scafs.path"`
    and `.fa`, with args.trim_info also `.tsv` and `.agp`; after a failure none of them is left.  -> (scaffolds, new paths).
    with_resident(scaffolds, resident): called once every file is written, while the contigs are still on the device (the merge
    stage goes on from there: merge.merge_after_overlap); its failure is the stage's."""
    import copy
    from . import anchor, gapfill
    if getattr(args, "v", False):
        raise ValueError("-v (the .mx.dot graph of every pair) is not available: no graph is built here")
    dev = dev or anchor._default_device()
    args = copy.copy(args)
    args.outgap = args.outgap + 1  # abyss-scaffold's path file counts one more
    try:
        with gapfill.resident_scaffolds(args.fasta, dev=dev, stitchable=True) as resident:
            scaffolds = read_fasta_file_trim_prep(resident)
            graph, _ = read_scaffold_graph(args.d)
            valid_mx_positions = find_valid_mx_regions(args, GAP_RE, graph, scaffolds)
            new_paths = merge_overlapping_pathfile(args, GAP_RE, graph, scaffolds, valid_mx_positions, dev=dev, resident=resident,
                                                   batch_bases=batch_bases)
            if args.trim_info:
                print_trim_coordinates(args, scaffolds)
                print_agp_file(new_paths, scaffolds, args)
            print_trimmed_scaffolds(args, scaffolds, resident=resident, dev=dev)
            if with_resident is not None:
                with_resident(scaffolds, resident)
    except BaseException:
        for suffix in OUTPUT_SUFFIXES:
            if os.path.exists(args.p + suffix):
                os.remove(args.p + suffix)
        raise
    return scaffolds, new_paths
