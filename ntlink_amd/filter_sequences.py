"""The sequences the overlap stage's sketch needs (bin/ntlink_filter_sequences.py, ntLink:246-248): per path line, the contigs that
have a valid minimizer region, in path order, then a `>LAST<path name>` record.

The FASTA file is resident as ASCII (gapfill.resident_scaffolds, stitchable); the valid regions come from
overlap.find_valid_mx_regions, which prints nothing; the output is one stitch plan -- a small store of header records, a copy
segment per printed contig, fill segments for the newlines -- assembled on the device and written in pieces through page-locked
memory (gapfill.write_stitched_records, the gap-fill writer).

The one difference from the reference: EVERY contig of the path file must be in the FASTA file, and this is checked before the
first byte is written.  The reference looks up only the contigs with a valid region, and fails with a KeyError in the middle of its
output."""
import re

from . import gapfill, overlap

GAP_RE = re.compile(r"^(\d+)N$")  # bin/ntlink_filter_sequences.py:15


def _records(path_file, valid_mx_regions, resident):
    "per output record: header bytes, segments, bytes of text (filter_sequences, :17-31)"
    for path_name, path_seq in overlap._path_lines(path_file, GAP_RE):
        for node in path_seq:
            if re.search(GAP_RE, node):
                continue
            name = node.strip("+-")
            if name in valid_mx_regions:  # once per occurrence
                rec = resident.number[name]
                length = int(resident.lengths[rec])
                header = f">{name}\n".encode()
                yield header, [(0, rec, 0, length, 0)] if length else [], len(header) + length + 1
        header = f">LAST{path_name}\nN".encode()
        yield header, [], len(header) + 1


def filter_sequences(args, out, dev=None, max_bytes=None):
    """main() of the reference behind its argument parser (:44-64).  args: fasta dot path k f g (t is not read).  out: a file name or
    a file descriptor open for writing.  Nothing is written when a contig of the path file is missing from the FASTA file."""
    from . import anchor
    dev = dev or anchor._default_device()
    graph, _ = overlap.read_scaffold_graph(args.dot)
    with gapfill.resident_scaffolds(args.fasta, dev=dev, stitchable=True) as resident:
        scaffolds = overlap.read_fasta_file_trim_prep(resident)
        for path_name, path_seq in overlap._path_lines(args.path, GAP_RE):
            for node in path_seq:
                if not re.search(GAP_RE, node) and node.strip("+-") not in scaffolds:
                    raise ValueError(f"path {path_name}: contig {node.strip('+-')} is not in the FASTA file")
        valid_mx_regions = overlap.find_valid_mx_regions(args, GAP_RE, graph, scaffolds)
        gapfill.write_stitched_records(dev, out, [resident.ascii], _records(args.path, valid_mx_regions, resident),
                                       max_bytes or gapfill.STITCH_BYTES)
    return valid_mx_regions
