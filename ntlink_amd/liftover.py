"""Liftover of the verbose mappings to the coordinates of the scaffolded sequences.

Same entry points as the reference's bin/ntlink_liftover_mappings.py (`read_agp` :39-50, `liftover_mappings`
:125-143, `main` :146-161); `read_agp` returns plain tuples of the columns the native call takes.  The per-line / per-read work (`liftover_ctg_mappings` :61-87, `print_adjusted_mappings`
:89-121) is native (csrc/ntl_liftover.cpp, `ntl_liftover` of include/ntlink_amd.h), several threads over pieces of the
file cut where the read id changes.  No GPU is involved.

`liftover_mappings_device` / `lift_result` are the device form (csrc/liftover_kernels.h, `ntl_mapres_liftover`): the same liftover of
a map result that is resident, or of the blocks of a file made resident, with the lines written by the device's formatter."""
import argparse
import ctypes as C
import os

import numpy as np

from . import capi


# columns of an AGP sequence line, in file order; ntl_liftover takes five of them
_AGP_COLUMNS = ("object", "object_beg", "object_end", "part_number", "component_type", "component_id", "component_beg",
                "component_end", "orientation")


def read_agp(agp_filename):
    """AGP file -> {contig id: (path id, scaf_start, ctg_start, ctg_end, orientation)}: the five columns `ntl_liftover`
    takes, one tuple per component (the last line of a contig id wins: the reference keeps a dict, read_agp :39-50).
    Gap lines (component type N or P) carry no contig and are left out; a line that does not have the nine AGP columns, or
    whose coordinates are not integers, raises ValueError (the reference fails on the same lines)."""
    table = {}
    with open(agp_filename, "r", encoding="utf-8") as fh:
        for lineno, line in enumerate(fh, 1):
            cols = line.strip().split("\t")
            if len(cols) != len(_AGP_COLUMNS):
                raise ValueError(f"{agp_filename}:{lineno}: {len(cols)} columns, an AGP line has {len(_AGP_COLUMNS)}")
            rec = dict(zip(_AGP_COLUMNS, cols))
            if rec["component_type"] in ("N", "P"):
                continue
            int(rec["object_end"]), int(rec["part_number"])  # the reference converts these too: same inputs fail
            table[rec["component_id"]] = (rec["object"], int(rec["object_beg"]), int(rec["component_beg"]),
                                          int(rec["component_end"]), rec["orientation"])
    return table


def _blob(strings):
    enc = [s.encode() for s in strings]
    off = np.zeros(len(enc) + 1, dtype=np.uint64)
    if enc:
        off[1:] = np.cumsum([len(b) for b in enc], dtype=np.uint64)
    return b"".join(enc), off


def liftover_mappings(mappings_filename, agp_dict, output, k):
    "Lifts <prefix>.verbose_mapping.tsv over to `output`; returns (lines read, lines written)"
    lib = capi.load()
    entries = list(agp_dict.items())
    ctg_blob, ctg_off = _blob([c for c, _ in entries])
    path_blob, path_off = _blob([e[0] for _, e in entries])
    scaf_start = np.array([e[1] for _, e in entries], dtype=np.int64)
    ctg_start = np.array([e[2] for _, e in entries], dtype=np.int64)
    ctg_end = np.array([e[3] for _, e in entries], dtype=np.int64)
    # only `+` and `-` move anything; every other orientation string means "leave the positions alone"
    ori = bytes((e[4].encode()[0] if len(e[4].encode()) == 1 else ord("?")) for _, e in entries)
    nin, nout = C.c_uint64(0), C.c_uint64(0)
    rc = lib.ntl_liftover(str(mappings_filename).encode(), str(output).encode(), int(k), len(entries),
                          ctg_blob, capi._ptr(ctg_off, C.c_uint64), path_blob, capi._ptr(path_off, C.c_uint64),
                          scaf_start.ctypes.data, ctg_start.ctypes.data, ctg_end.ctypes.data, ori, C.byref(nin), C.byref(nout))
    if rc == capi.NTL_EINVAL:
        raise ValueError(f"liftover of {mappings_filename}: unreadable file or malformed line "
                         "(expected read<TAB>contig<TAB>count<TAB>ctgpos:strand_readpos:strand ...)")
    if rc:
        raise capi.NtlError(f"ntl_liftover failed ({rc})")
    return nin.value, nout.value


def lift_table(agp_dict, contig_names):
    """The entry table of `ntl_mapres_liftover` over `contig_names` (the INPUT name space: entry i belongs to contig_names[i]) and the
    list of OUTPUT names: the distinct path ids and the names of the contigs that are not in the AGP, in order of first appearance
    (an absent contig keeps its name, which may be a path id as well: one output name).  "path id == contig id" -- such a component
    is left where it is, whatever its orientation (:75-84) -- is decided here, on strings.  -> (capi.LIFT_ENTRY_DT array, list of str)"""
    out_names, number = [], {}
    table = np.zeros(len(contig_names), capi.LIFT_ENTRY_DT)
    for i, ctg in enumerate(contig_names):
        entry = agp_dict.get(ctg)
        name = ctg if entry is None else entry[0]
        if name not in number:
            number[name] = len(out_names)
            out_names.append(name)
        if entry is None:
            table[i] = (number[name], capi.NTL_LIFT_ABSENT, 0, 0, 0)
            continue
        path, scaf_start, ctg_start, ctg_end, ori = entry
        for v in (scaf_start, ctg_start, ctg_end):
            if not 0 <= v <= 0xFFFFFFFF:
                raise ValueError(f"AGP component {ctg}: coordinate {v} is outside 0 .. 2^32 - 1")
        mode = capi.NTL_LIFT_KEEP if path == ctg or ori not in ("+", "-") else capi.NTL_LIFT_SHIFT if ori == "+" else capi.NTL_LIFT_MIRROR
        table[i] = (number[name], mode, scaf_start, ctg_start, ctg_end)
    return table, out_names


def lift_result(result, agp_dict, contig_names, k, dev):
    """A resident capi.MapResult whose contig numbers index `contig_names`, lifted through the AGP on the device.  -> (the new
    MapResult, the output names its contig numbers index).  `result` is completed and left alone.  The next round's tally of the lifted
    result needs none of its records on the host: dev.mapres_pairs(lifted, dev.pair_table(tally)) with a PairTally over the output
    names gives the pair records (read_len=None: the checkpoint rule), and tally.add_pairs takes them."""
    table, out_names = lift_table(agp_dict, contig_names)
    return dev.mapres_liftover(result, table, k), out_names


def _unknown_contig(mappings_filename, known):
    "the first contig name of the file that is not in `known` (the error path of liftover_mappings_device)"
    with open(mappings_filename, "rb") as fh:
        for line in fh:
            cols = line.split(b"\t")
            if len(cols) > 1 and cols[1].decode(errors="replace") not in known:
                return cols[1].decode(errors="replace")
    return "?"


def liftover_mappings_device(mappings_filename, agp_dict, output, k, dev, contig_names=None, tally=None, max_bytes=256 << 20,
                             device_tally=False):
    """`liftover_mappings` on the device `dev` (capi.Device): blocks of whole reads of about max_bytes of text (formats.read_verbose)
    become resident results (mapres_from_host), are lifted there (mapres_liftover), and the lines the device's formatter makes of them
    are written block by block (ntl_write_blob) to a temporary file beside `output`, which takes its name when it is complete; on
    failure no file is left.  -> (lines read, lines written); the bytes are those of `liftover_mappings`.

    contig_names: the input name space -- by default the AGP's contig ids; a caller who knows of contigs that are not in the AGP
    (sequences the overlap stage left out, say) lists them too.  tally: a pairing.PairTally over the OUTPUT names (lift_table gives
    them): every block's mappings and first / last hits go to it as well (ntl_tally_add_ends, the read length being the largest mapped
    read position as in the checkpoint path, bin/ntlink_pair.py:460-488) -- the next round's tally without reading the lifted file.
    device_tally: with `tally`, the lifted result's pair records are made on the device instead (Device.mapres_pairs with
    read_len=None, which is that rule) and the tally takes them with add_pairs: the same tally.

    Two differences from the host path, which never parses the tokens of a contig that is not in the AGP and needs no name table:
    a line that names a contig which is neither in the AGP nor in contig_names raises ValueError naming it, and a malformed token
    on ANY line raises ValueError."""
    from . import formats
    names = list(agp_dict) if contig_names is None else list(contig_names)
    table, out_names = lift_table(agp_dict, names)
    tmp = f"{output}.tmp{os.getpid()}"
    lines_in = lines_out = 0
    no_pafs = np.zeros(0, capi.PAF_DT)
    fd = os.open(tmp, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
    pair_tab = dev.pair_table(tally) if tally is not None and device_tally else None
    try:
        with dev.names(out_names, np.zeros(len(out_names), np.uint32)) as cn:
            for block in formats.read_verbose(str(mappings_filename), names, max_bytes=max_bytes, lib_path=dev.lib_path):
                if len(block.maps) and int(block.maps["ctg"].max()) == capi.NO_CTG:
                    raise ValueError(f"liftover of {mappings_filename}: contig {_unknown_contig(mappings_filename, set(names))} is neither in the "
                                     "AGP nor in contig_names")
                lines_in += len(block.maps)
                n_reads = len(block.map_off) - 1
                with dev.mapres_from_host(block.maps, block.hits, no_pafs) as res, dev.mapres_liftover(res, table, k) as lifted, \
                        dev.names(block.names, np.zeros(n_reads, np.uint32)) as rn, lifted.format(rn, cn, True, False) as text:
                    d = text.download()
                    recs = dev.mapres_pairs(lifted, pair_tab) if pair_tab is not None else None
                try:
                    if len(d["verbose"]) and dev.L.ntl_write_blob(fd, d["verbose"].ctypes.data, len(d["verbose"])) != 0:
                        raise OSError(f"writing {tmp} failed")
                    lines_out += len(d["maps"])
                    if recs is not None:
                        tally.add_pairs(recs)
                    elif tally is not None and len(d["maps"]):
                        read_len = np.zeros(n_reads, np.uint32)
                        np.maximum.at(read_len, d["maps"]["read"], np.maximum(d["ends"]["read_pos"][0::2], d["ends"]["read_pos"][1::2]))
                        tally.add_batch_ends(d["maps"], d["ends"], read_len)
                finally:
                    dev.pinned_release(d["_pinned"])
        os.close(fd)
        fd = None
        os.replace(tmp, output)
    except BaseException:
        if fd is not None:
            os.close(fd)
        if os.path.exists(tmp):
            os.remove(tmp)
        raise
    finally:
        if pair_tab is not None:
            pair_tab.close()
    return lines_in, lines_out


def main(argv=None):
    "Liftover the ntLink verbose mappings file (arguments of bin/ntlink_liftover_mappings.py:146-153)"
    parser = argparse.ArgumentParser(description="Liftover of ntLink mappings")
    parser.add_argument("-m", "--mappings", help="Path to the verbose mappings file", required=True)
    parser.add_argument("-a", "--agp", help="Path to the AGP file", required=True)
    parser.add_argument("-o", "--output", help="Output file name", required=True)
    parser.add_argument("-k", "--kmer", help="Kmer size", required=True, type=int)
    parser.add_argument("--device", help="Lift on this GPU (HIP ordinal) instead of on the host", type=int, default=None, metavar="ORDINAL")
    parser.add_argument("--contigs", help="With --device: FASTA of the sequences the mappings name (those that are not in the AGP keep "
                        "their names and lose their mappings)", default=None, metavar="FASTA")
    from .cli import VERSION
    parser.add_argument("-v", "--version", action="version", version=VERSION)
    args = parser.parse_args(argv)
    if args.device is None:
        if args.contigs is not None:
            parser.error("--contigs needs --device")
        liftover_mappings(args.mappings, read_agp(args.agp), args.output, args.kmer)
        return 0
    agp = read_agp(args.agp)
    names = None
    if args.contigs is not None:
        from . import seqio
        names = seqio.load_all([args.contigs]).names.tolist()
        listed = set(names)
        names += [c for c in agp if c not in listed]
    dev = capi.Device(args.device)
    try:
        liftover_mappings_device(args.mappings, agp, args.output, args.kmer, dev, contig_names=names)
    finally:
        dev.close()
    return 0
