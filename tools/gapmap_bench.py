#!/usr/bin/env python3
"""The gap filler's re-mapping loop, grouped against per gap (not the flagship benchmark).

For G synthetic gaps (two scaffold ends of 300 .. 3000 bases, one read piece across them with 5 % errors, k20 w10), in one process:
  grouped   gapfill.map_gap_sequences: sketch, ONE ntl_map_run_grouped, records to Python objects
  per_gap   what the library offered before: one anchor.get_accepted_anchor_contigs per gap (a sketch upload, an index build, a second
            upload, a map and a download each) from the same sketches' arrays, over the first 2000 gaps, scaled to G
  kernel    group_probe_kernel alone (ntl_prof_get "probe") beside the bytes it moves: 16 B per contig record and per read record in,
            12 B per read record out
  cuts      (--cuts) the whole of the reference's map_long_reads over the two temporary files, best of --repeat in one process:
            gapfill.map_long_reads (the cuts decided by gap_cut_kernel: 32 B per gap come back) beside the way to the same answer before
            it -- gapfill.map_gap_reads and assess_accepted_anchor_contigs (bin/ntlink_patch_gaps.py:443-517) in Python over its Gap
            objects; both end states must be equal.  Also gap_cut_kernel alone (ntl_prof_get "gap_cut") and the bytes it reads: per gap
            two offsets, two signs and, with two mappings, their two records and 12 B per hit.
  select    (--select) the choice of every gap's read from the verbose mappings: a synthetic <prefix>.verbose_mapping.tsv of G gaps with
            about 30 supporting reads each and ten times as many reads that support nothing, written by formats.write_verbose; best of
            --repeat in one process: gapfill.choose_gap_reads, gapfill.choose_gap_reads_restated (the reference's three functions in
            Python; both must leave the same fields in every pair), the three kernels of ntl_gap_select alone (ntl_prof_get
            "gap_select": assess, count, scan with its host wait, fill) beside the bytes the block uploads, and the reader alone in
            GB/s of text.
  mask      (--mask) from the chosen reads to the final cuts, with and without the two temporary files: a chain of G + 1 scaffolds of
            --scaffold-len bases (50 kb: 2 G records of that length are written, 0.2 GB at 2 000 gaps and 2 GB at 20 000), per gap a read
            of 1 .. 6 kb whose middle spans the gap with 5 % errors, random signs; best of --repeat, alternating:
            (a) gapfill.print_masked_sequences (timed as `write_s`) and gapfill.map_long_reads over the two files (`read_s`),
            (b) gapfill.map_long_reads_resident over the resident scaffolds and reads (`resident_s`; making the two resident batches
            once is `setup_s`), with the batch_mask kernels' share (ntl_prof_get "batch_mask") from one more run.  Both must leave the
            same fields in every pair and scaffold.
Prints one JSON line per G (and one per G for --cuts / --select / --mask)."""
import argparse
import json
import sys
import os
import tempfile
import time
import types

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ntlink_amd import anchor, capi, formats, gapfill  # noqa: E402

ACGT = np.frombuffer(b"ACGT", np.uint8)
K, W = 20, 10


def make_gaps(n, seed=1):
    rng = np.random.default_rng(seed)
    scaffolds, reads = [], []
    for g in range(n):
        src, tgt = ACGT[rng.integers(0, 4, int(rng.integers(300, 3001)))], ACGT[rng.integers(0, 4, int(rng.integers(300, 3001)))]
        piece = np.concatenate([src[-int(rng.integers(250, 900)):], ACGT[rng.integers(0, 4, int(rng.integers(50, 400)))],
                                tgt[:int(rng.integers(250, 900))]])
        hit = rng.random(len(piece)) < 0.05
        piece[hit] = ACGT[rng.integers(0, 4, int(hit.sum()))]
        scaffolds += [(f"s{2 * g}+_source", b"N" * int(rng.integers(0, 500)) + src.tobytes()),
                      (f"s{2 * g + 1}+_target", tgt.tobytes() + b"N" * int(rng.integers(0, 500)))]
        reads.append((f"r{g}__s{2 * g}+__s{2 * g + 1}+", piece.tobytes()))
    return scaffolds, reads


def per_gap_loop(dev, scaffolds, reads, args, n):
    """the per-gap way over the first n gaps; the sketches are made once, as for the grouped pass, and are not timed"""
    with dev.batch([s for _i, s in scaffolds[:2 * n]]) as sb, dev.batch([s for _i, s in reads[:n]]) as rb, \
            dev.sketch(sb, K, W) as ssk, dev.sketch(rb, K, W) as rsk:
        soff, sh, sp, ss = ssk.download()
        roff, rh, rp, rs = rsk.download()
    names = [gapfill.default_name_of(i) for i, _s in scaffolds[:2 * n]]
    lens = {names[i]: gapfill._Length(len(scaffolds[i][1])) for i in range(2 * n)}
    two = 0
    t0 = time.perf_counter()
    for g in range(n):
        mx_info, dup = {}, set()
        for c in (2 * g, 2 * g + 1):
            for j in range(int(soff[c]), int(soff[c + 1])):
                key = str(int(sh[j]))
                if key in mx_info:
                    dup.add(key)
                else:
                    mx_info[key] = anchor.Minimizer(names[c], int(sp[j]), "+" if ss[j] else "-")
        for key in dup:
            del mx_info[key]
        mxs = [(str(int(rh[j])), int(rp[j]), "+" if rs[j] else "-") for j in range(int(roff[g]), int(roff[g + 1])) if str(int(rh[j])) in mx_info]
        accepted, _order = anchor.get_accepted_anchor_contigs(mxs, len(reads[g][1]), lens, mx_info, args, dev=dev)
        two += len(accepted) == 2
    return time.perf_counter() - t0, two


def host_map_long_reads(pairs, scaffolds, args, dev):
    """map_long_reads before gap_cut_kernel: every hit downloaded and made an object, then :443-517 in Python"""
    k = args.k
    gaps = gapfill.map_gap_reads(args.o + ".scaffolds.masked_temp.fa", args.o + ".reads.masked_temp.fa", args.k, args.w, args, dev=dev)
    for gap in gaps:
        _, source, target = gap.read.id.split("__")
        sname, tname = source.strip("+-"), target.strip("+-")
        pair = pairs[(source, target)]
        sides = None
        if len(gap.accepted) == 2:
            sides = []
            for name, sign, source_side in ((sname, source[-1], True), (tname, target[-1], False)):
                hits = gap.accepted[name].hits
                if all(h.ctg_strand == h.read_strand for h in hits):
                    ori = "+"
                elif all(h.ctg_strand != h.read_strand for h in hits):
                    ori = "-"
                else:
                    ori = None
                consistent = all(a.ctg_pos < b.ctg_pos for a, b in zip(hits, hits[1:])) or all(a.ctg_pos > b.ctg_pos for a, b in zip(hits, hits[1:]))
                if ori is None or not consistent:
                    sides = None
                    break
                t = hits[-1 if (sign == ori) == source_side else 0]
                sides.append((t.ctg_pos, t.read_pos + k if ori != sign and sign == "+" else t.read_pos,
                              t.ctg_pos + k if ori == sign and sign == "-" else t.ctg_pos))
        if sides is None:
            if args.stringent:
                pair.source_read_cut = pair.target_read_cut = None
            else:
                gapfill._fallback_old_anchor_cuts(pair, scaffolds, sname, source[-1] == "-", tname, target[-1] == "-")
            continue
        pair.source_ctg_cut, pair.source_read_cut, pair.target_ctg_cut, pair.target_read_cut = sides[0][0], sides[0][1], sides[1][0], sides[1][1]
        setattr(scaffolds[sname], "three_prime_cut" if source[-1] == "+" else "five_prime_cut", sides[0][2])
        setattr(scaffolds[tname], "five_prime_cut" if target[-1] == "+" else "three_prime_cut", sides[1][2])


def cuts_leg(dev, G, repeat):
    scaffolds, reads = make_gaps(G)
    rng = np.random.default_rng(G)
    for g in range(G):  # random signs, every other read against the path
        s, t = "+-"[int(rng.integers(0, 2))], "+-"[int(rng.integers(0, 2))]
        scaffolds[2 * g] = (f"s{2 * g}{s}_source", scaffolds[2 * g][1])
        scaffolds[2 * g + 1] = (f"s{2 * g + 1}{t}_target", scaffolds[2 * g + 1][1])
        seq = reads[g][1]
        reads[g] = (f"r{g}__s{2 * g}{s}__s{2 * g + 1}{t}", seq.translate(bytes.maketrans(b"ACGT", b"TGCA"))[::-1] if g & 1 else seq)

    def fresh():
        pairs = {tuple(rid.split("__")[1:]): types.SimpleNamespace(source_ctg_cut=1, source_read_cut=2, target_ctg_cut=3, target_read_cut=4,
                                                                   old_anchor_used=False) for rid, _s in reads}
        scaf = {sid.rsplit("_", 1)[0].strip("+-"): types.SimpleNamespace(five_prime_cut=0, three_prime_cut=len(seq)) for sid, seq in scaffolds}
        return pairs, scaf

    with tempfile.TemporaryDirectory() as tmp:
        prefix = os.path.join(tmp, "g")
        for suffix, recs in ((".scaffolds.masked_temp.fa", scaffolds), (".reads.masked_temp.fa", reads)):
            with open(prefix + suffix, "wb") as fh:
                for rid, seq in recs:
                    fh.write(b">" + rid.encode() + b"\n" + seq + b"\n")
        args = argparse.Namespace(o=prefix, k=K, w=W, z=1000, x=0.0, sensitive=False, stringent=False)
        gapfill.map_long_reads(*fresh(), args, dev=dev)  # warm-up
        t_new, t_old, states = [], [], []
        for fn, times in ((gapfill.map_long_reads, t_new), (host_map_long_reads, t_old)):
            for _ in range(repeat):
                pairs, scaf = fresh()
                t0 = time.perf_counter()
                fn(pairs, scaf, args, dev)
                times.append(time.perf_counter() - t0)
            states.append(([vars(p) for p in pairs.values()], {n: vars(s) for n, s in scaf.items()}))
        assert states[0] == states[1], "the two ways leave different cuts"
    # the kernel alone: one stream, events round it
    dev.set_pipeline(False)
    dev.prof_enable(True)
    dev.prof_reset()
    minus = np.zeros(G, np.uint8)
    with dev.batch([s for _i, s in scaffolds]) as sb, dev.batch([s for _i, s in reads]) as rb, dev.sketch(sb, K, W) as ssk, dev.sketch(rb, K, W) as rsk:
        clen = np.array([len(s) for _i, s in scaffolds], np.uint32); rlen = np.array([len(s) for _i, s in reads], np.uint32)
        with dev.map_grouped(ssk, clen, 2 * np.arange(G + 1, dtype=np.uint32), rsk, rlen, np.arange(G + 1, dtype=np.uint32), k=K) as res:
            for _ in range(repeat):
                cuts = res.gap_cuts(minus, minus, K)
            maps = res.download()["maps"]
    ms, launches = dev.prof_get("gap_cut")
    dev.prof_enable(False)
    dev.set_pipeline(True)
    two = np.flatnonzero(np.bincount(maps["read"], minlength=G) == 2)
    read_bytes = 10 * G + int(np.isin(maps["read"], two).sum()) * 24 + 12 * int(maps["n_hits"][np.isin(maps["read"], two)].sum())
    kernel_ms = ms / max(1, launches)
    new_cuts = sum(not p["old_anchor_used"] for p in states[0][0])
    print(json.dumps({"leg": "cuts", "gaps": G, "map_long_reads_s": min(t_new), "map_long_reads_s_all": t_new, "host_assess_s": min(t_old),
                      "host_assess_s_all": t_old, "ratio": min(t_old) / min(t_new), "new_cuts": new_cuts, "valid_status": int((cuts["status"] == 0).sum()),
                      "gap_cut_kernel_ms": kernel_ms, "gap_cut_read_bytes": read_bytes, "gap_cut_GBps": read_bytes / kernel_ms / 1e6 if kernel_ms else None,
                      "device": dev.name}), flush=True)


def make_verbose(path, G, per_gap=30, idle=10, seed=3):
    """G + 1 contigs in a chain of G gaps; per gap `per_gap` reads that map to its two contigs in a row (3 .. 12 hits each, near the
    gap) and per_gap * idle reads with one mapping somewhere; in random order, written by the project's emitter.  -> path text, lengths"""
    rng = np.random.default_rng(seed)
    LEN = 20000
    n_sup, n_idle = G * per_gap, G * per_gap * idle
    n_reads = n_sup + n_idle
    is_sup = np.zeros(n_reads, bool)
    is_sup[rng.permutation(n_reads)[:n_sup]] = True
    gap_of = rng.integers(0, G, n_reads)
    per_read = np.where(is_sup, 2, 1)
    first = np.concatenate([[0], np.cumsum(per_read)])
    n_maps = int(first[-1])
    maps = np.zeros(n_maps, capi.MAPPING_DT)
    maps["read"] = np.repeat(np.arange(n_reads), per_read)
    second = np.zeros(n_maps, bool)
    second[first[:-1][is_sup] + 1] = True
    maps["ctg"] = np.repeat(gap_of, per_read) + second
    maps["n_hits"] = rng.integers(3, 13, n_maps)
    off = np.concatenate([[0], np.cumsum(maps["n_hits"])])
    maps["hit_off"] = off[:-1]
    idx = np.arange(int(off[-1])) - np.repeat(off[:-1], maps["n_hits"])
    hits = np.zeros(int(off[-1]), capi.HIT_DT)
    c0 = np.where(second, 100, LEN - 700)  # a source ends near its contig's end, a target starts near its start
    hits["ctg_pos"] = np.repeat(c0, maps["n_hits"]) + 50 * idx
    hits["read_pos"] = np.repeat(np.where(second, 2000, 1000), maps["n_hits"]) + 40 * idx
    hits["ctg_strand"] = hits["read_strand"] = 1
    with open(path, "w") as fh:
        formats.write_verbose(fh, {"maps": maps, "hits": hits}, [f"r{i}" for i in range(n_reads)], [f"c{i}" for i in range(G + 1)])
    return "".join(f"p{g}\tc{g}+ 500N c{g + 1}+\n" for g in range(G)), {f"c{i}": types.SimpleNamespace(length=LEN) for i in range(G + 1)}, int(off[-1])


def select_leg(dev, G, repeat):
    with tempfile.TemporaryDirectory() as tmp:
        vp, pp = os.path.join(tmp, "g.verbose_mapping.tsv"), os.path.join(tmp, "g.path")
        path_text, sequences, n_hits = make_verbose(vp, G)
        with open(pp, "w") as fh:
            fh.write(path_text)
        text_bytes = os.path.getsize(vp)
        args = argparse.Namespace(large_k=K)
        state = lambda pairs: [(sorted(p.mapping_reads), p.chosen_read, p.source_ctg_cut, p.source_read_cut, p.target_ctg_cut, p.target_read_cut)
                               for p in pairs.values()]
        gapfill.choose_gap_reads(gapfill.read_path_file_pairs(pp, 20), vp, sequences, args, dev=dev)  # warm-up
        t_new, t_old, states = [], [], []
        for fn, times in ((lambda p: gapfill.choose_gap_reads(p, vp, sequences, args, dev=dev), t_new),
                          (lambda p: gapfill.choose_gap_reads_restated(p, vp, sequences, args), t_old)):
            for _ in range(repeat):
                pairs = gapfill.read_path_file_pairs(pp, 20)
                t0 = time.perf_counter()
                fn(pairs)
                times.append(time.perf_counter() - t0)
            states.append(state(pairs))
        assert states[0] == states[1], "the two ways leave different fields"
        ctg_names, ctg_len, keys = gapfill.pair_tables(gapfill.read_path_file_pairs(pp, 20), sequences)
        t_read = []
        for _ in range(repeat):
            t0 = time.perf_counter()
            blocks = list(formats.read_verbose(vp, ctg_names, max_bytes=gapfill.VERBOSE_BLOCK_BYTES))
            t_read.append(time.perf_counter() - t0)
        table = capi.pair_table(keys)
        dev.set_pipeline(False)
        dev.prof_enable(True)
        dev.prof_reset()
        t_call, n_cand = [], 0
        for _ in range(repeat):
            t0 = time.perf_counter()
            n_cand = sum(len(dev.gap_select(b, ctg_len, K, table)) for b in blocks)
            t_call.append(time.perf_counter() - t0)
        ms, launches = dev.prof_get("gap_select")
        dev.prof_enable(False)
        dev.set_pipeline(True)
        up = sum(b.map_off.nbytes + b.maps.nbytes + b.anchors.nbytes + b.hits.nbytes for b in blocks) + len(blocks) * (ctg_len.nbytes + 12 * len(table[0]))
        kernel_ms = ms / max(1, launches) * len(blocks)
        print(json.dumps({"leg": "select", "gaps": G, "reads": sum(len(b.names) for b in blocks), "hits": n_hits, "text_bytes": text_bytes,
                          "blocks": len(blocks), "candidates": n_cand, "chosen": sum(s[1] is not None for s in states[0]),
                          "choose_gap_reads_s": min(t_new), "choose_gap_reads_s_all": t_new, "restated_s": min(t_old), "restated_s_all": t_old,
                          "ratio": min(t_old) / min(t_new), "reader_s": min(t_read), "reader_GBps": text_bytes / min(t_read) / 1e9,
                          "gap_select_call_s": min(t_call), "gap_select_kernels_ms": kernel_ms, "upload_bytes": up,
                          "kernels_GBps_of_upload": up / kernel_ms / 1e6 if kernel_ms else None, "device": dev.name}), flush=True)


def mask_leg(dev, G, repeat, scaffold_len):
    rng = np.random.default_rng(G)
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    blob = ACGT[rng.integers(0, 4, (G + 1) * scaffold_len, dtype=np.uint8)].tobytes()
    seqs = {f"c{i}": blob[i * scaffold_len:(i + 1) * scaffold_len] for i in range(G + 1)}
    del blob
    reads, spec = {}, []
    for g in range(G):
        s, t = "+-"[int(rng.integers(0, 2))], "+-"[int(rng.integers(0, 2))]
        rs, rt = int(rng.integers(250, 900)), int(rng.integers(250, 900))
        src, tgt = seqs[f"c{g}"], seqs[f"c{g + 1}"]
        end = src[-rs:] if s == "+" else src[:rs].translate(comp)[::-1]
        start = tgt[:rt] if t == "+" else tgt[-rt:].translate(comp)[::-1]
        piece = np.frombuffer(end + ACGT[rng.integers(0, 4, int(rng.integers(50, 400)))].tobytes() + start, np.uint8).copy()
        hit = rng.random(len(piece)) < 0.05
        piece[hit] = ACGT[rng.integers(0, 4, int(hit.sum()))]
        pre, post = (ACGT[rng.integers(0, 4, int(rng.integers(0, 2500)))].tobytes() for _ in range(2))
        read = pre + piece.tobytes() + post
        cuts = (len(pre), len(pre) + len(piece))
        if g & 1:  # every other read against the path
            read, cuts = read.translate(comp)[::-1], (len(read) - cuts[0], len(read) - cuts[1])
        reads[f"r{g}"] = read
        keep_s, keep_t = int(rng.integers(rs, 3001)), int(rng.integers(rt, 3001))
        spec.append((f"c{g}{s}", f"c{g + 1}{t}", scaffold_len - keep_s if s == "+" else keep_s, cuts[0],
                     keep_t if t == "+" else scaffold_len - keep_t, cuts[1]))

    def fresh():
        pairs = {}
        for g, (source, target, sc, sr, tc, tr) in enumerate(spec):
            p = gapfill.PairInfo(100)
            p.chosen_read, p.source_ctg_cut, p.source_read_cut, p.target_ctg_cut, p.target_read_cut = f"r{g}", sc, sr, tc, tr
            pairs[(source, target)] = p
        return pairs, {name: types.SimpleNamespace(five_prime_cut=0, three_prime_cut=scaffold_len) for name in seqs}

    state = lambda pairs, scaf: ([vars(p) for p in pairs.values()], {n: vars(x) for n, x in scaf.items()})
    t0 = time.perf_counter()
    res_s, res_r = gapfill.resident_scaffolds(seqs.items(), dev=dev), gapfill.resident_scaffolds(reads.items(), dev=dev)
    dev.sync()
    t_setup = time.perf_counter() - t0
    t_write, t_read, t_res, states = [], [], [], []
    with tempfile.TemporaryDirectory() as tmp:
        args = argparse.Namespace(o=os.path.join(tmp, "g"), k=K, w=W, z=1000, x=0.0, sensitive=False, stringent=False)
        gapfill.map_long_reads_resident(*fresh(), res_s, res_r, args, dev=dev)  # warm-up
        for _ in range(repeat):
            pairs, scaf = fresh()
            t0 = time.perf_counter()
            gapfill.print_masked_sequences(seqs, reads, pairs, args)
            t1 = time.perf_counter()
            gapfill.map_long_reads(pairs, scaf, args, dev=dev)
            t2 = time.perf_counter()
            t_write.append(t1 - t0); t_read.append(t2 - t1)
            states.append(state(pairs, scaf))
            pairs, scaf = fresh()
            t0 = time.perf_counter()
            gapfill.map_long_reads_resident(pairs, scaf, res_s, res_r, args, dev=dev)
            t_res.append(time.perf_counter() - t0)
            states.append(state(pairs, scaf))
        text_bytes = os.path.getsize(args.o + ".scaffolds.masked_temp.fa") + os.path.getsize(args.o + ".reads.masked_temp.fa")
        assert all(st == states[0] for st in states), "the two ways leave different cuts"
        dev.set_pipeline(False)
        dev.prof_enable(True)
        dev.prof_reset()
        gapfill.map_long_reads_resident(*fresh(), res_s, res_r, args, dev=dev)
        dev.sync()
        ms, launches = dev.prof_get("batch_mask")
        dev.prof_enable(False)
        dev.set_pipeline(True)
    res_s.close(); res_r.close()
    new_cuts = sum(not p["old_anchor_used"] for p in states[0][0])
    print(json.dumps({"leg": "mask", "gaps": G, "scaffold_len": scaffold_len, "text_bytes": text_bytes, "write_s": min(t_write), "write_s_all": t_write,
                      "read_s": min(t_read), "read_s_all": t_read, "resident_s": min(t_res), "resident_s_all": t_res, "setup_s": t_setup,
                      "read_over_resident": min(t_read) / min(t_res), "files_over_resident": (min(t_write) + min(t_read)) / min(t_res),
                      "new_cuts": new_cuts, "batch_mask_ms": ms, "batch_mask_spans": launches, "device": dev.name}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaps", type=int, nargs="+", default=[2000, 20000])
    ap.add_argument("--per-gap", type=int, default=2000, help="gaps the per-gap loop runs over (scaled to G)")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--cuts", action="store_true", help="the cuts leg alone: gapfill.map_long_reads beside map_gap_reads + the assess in Python")
    ap.add_argument("--select", action="store_true", help="the select leg alone: gapfill.choose_gap_reads beside the three reference functions in Python")
    ap.add_argument("--mask", action="store_true", help="the mask leg alone: the two temporary files written and read beside gapfill.map_long_reads_resident")
    ap.add_argument("--scaffold-len", type=int, default=50000, help="bases per scaffold of the mask leg")
    a = ap.parse_args()
    args = argparse.Namespace(k=K, z=1000, x=0.0, sensitive=False)
    dev = capi.Device(0)
    if a.mask:
        for G in a.gaps:
            mask_leg(dev, G, a.repeat, a.scaffold_len)
        dev.close()
        return
    if a.select:
        for G in a.gaps:
            select_leg(dev, G, a.repeat)
        dev.close()
        return
    if a.cuts:
        for G in a.gaps:
            cuts_leg(dev, G, a.repeat)
        dev.close()
        return
    for G in a.gaps:
        scaffolds, reads = make_gaps(G)
        list(gapfill.map_gap_sequences(scaffolds[:200], reads[:100], K, W, args, dev=dev))  # warm-up: code objects, pools
        times = []
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            two = sum(len(g.accepted) == 2 for g in gapfill.map_gap_sequences(scaffolds, reads, K, W, args, dev=dev))
            times.append(time.perf_counter() - t0)
        # the kernel alone: one stream, events round the lookup
        dev.set_pipeline(False)
        dev.prof_enable(True)
        dev.prof_reset()
        with dev.batch([s for _i, s in scaffolds]) as sb, dev.batch([s for _i, s in reads]) as rb, dev.sketch(sb, K, W) as ssk, dev.sketch(rb, K, W) as rsk:
            n_c, n_r = ssk.count, rsk.count
            clen = np.array([len(s) for _i, s in scaffolds], np.uint32); rlen = np.array([len(s) for _i, s in reads], np.uint32)
            for _ in range(a.repeat):
                with dev.map_grouped(ssk, clen, 2 * np.arange(G + 1, dtype=np.uint32), rsk, rlen, np.arange(G + 1, dtype=np.uint32), k=K) as res:
                    res.wait()
                    info = res.grouped_info
        probe_ms, launches = dev.prof_get("probe")
        dev.prof_enable(False)
        dev.set_pipeline(True)
        n_pg = min(a.per_gap, G)
        t_pg, two_pg = per_gap_loop(dev, scaffolds, reads, args, n_pg)
        kernel_ms = probe_ms / max(1, launches)
        moved = 16 * n_c + 16 * n_r + 12 * n_r
        print(json.dumps({"gaps": G, "grouped_s": min(times), "grouped_s_all": times, "per_gap_s_scaled": t_pg * G / n_pg, "per_gap_gaps_run": n_pg,
                          "ratio": t_pg * G / n_pg / min(times), "two_accepted": two, "two_accepted_per_gap": two_pg,
                          "probe_kernel_ms": kernel_ms, "probe_bytes": moved, "probe_GBps": moved / kernel_ms / 1e6,
                          "contig_records": n_c, "read_records": n_r, "grouped_info": info, "device": dev.name}), flush=True)
    dev.close()


if __name__ == "__main__":
    main()
