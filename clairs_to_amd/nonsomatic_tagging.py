"""`python -m clairs_to_amd nonsomatic_tagging ...` - the reference's src/nonsomatic_tagging.py (STEP 3 / STEP 7 of run_clairs_to) with the
panel-of-normals scan on the device (csrc/pon.hip, cto_pon_*).

What stays on the host: reading the pileup VCF (shared/vcf.py:VcfReader as nonsomatic_tagging calls it), the md5 of every PoN (hashlib on a
thread of its own, while the device scans the same file), the lines the device hands back (parsed here by the reference's line rule,
pon_record), the header, the rows and the summaries.  Output is the reference's byte for byte (tests/test_gpu_nonsomatic.py)."""
import argparse
import ctypes as C
import fcntl
import hashlib
import os
import sys
import threading
from collections import OrderedDict

from . import _cli

major_contigs_order = ["chr" + str(a) for a in list(range(1, 23)) + ["X", "Y"]] + [str(a) for a in list(range(1, 23)) + ["X", "Y"]]
REFCALL_FILTER_LINE = '##FILTER=<ID=RefCall,Description="Reference call">'


# ------------------------------------------------------------------------------------------ input
def read_pileup_vcf(fn, ctg_name, show_ref, filter_tag):
    """shared/vcf.py:VcfReader(keep_row_str=True, save_header=True).read_vcf() as nonsomatic_tagging uses it -> (header, {key: call}) with
    key = POS (ctg_name set) or (CHROM, POS), call = dict(ctg, pos, ref, alt (first ALT), filter, row); a later row at the same key replaces
    an earlier one, as the reference's dict does."""
    import gzip
    header, calls = "", {}
    if fn is None or not os.path.exists(fn):
        return header, calls
    with open(fn, "rb") as f:
        gz = f.read(2) == b"\x1f\x8b"
    fo = gzip.open(fn, "rt") if gz else open(fn)
    if ctg_name is None:
        only, tuple_keys = None, True
    elif "," in ctg_name:
        only, tuple_keys = frozenset(x.strip() for x in ctg_name.split(",") if x.strip()), True
    else:
        only, tuple_keys = frozenset([ctg_name]), False
    allowed = None if filter_tag is None else filter_tag.split(",")
    with fo:
        for row in fo:
            columns = row.strip().split()
            if columns[0][0] == "#":
                header += row
                continue
            chromosome, position = columns[0], columns[1]
            if only is not None and chromosome not in only:
                continue
            flt = columns[6] if len(columns) >= 7 else None
            if allowed is not None and flt not in allowed:
                continue
            reference, alternate = columns[3], columns[4]
            genotype = columns[-1].split(":")[0].replace("/", "|").replace(".", "0").split("|")
            try:
                g1, g2 = genotype
                if int(g1) > int(g2):
                    g1, g2 = g2, g1
                if "*" in alternate:
                    alts = alternate.split(",")
                    if int(g1) + int(g2) != 3 or len(alts) != 2:
                        print("error with variant representation")
                        continue
                    alternate = "".join(a for a in alts if a != "*")
                    g1, g2 = "0", "1"
            except Exception:
                g1 = g2 = -1
            position = int(position)
            if g1 == "0" and g2 == "0" and not show_ref:
                continue
            key = (chromosome, position) if tuple_keys else position
            calls[key] = dict(ctg=chromosome, pos=position, ref=reference, alt=alternate.split(",")[0], filter=flt, row=row)
    return header, calls


def call_sets(calls, ctg_name, show_ref):
    """-> OrderedDict contig -> {pos: call} of the calls that take part (PASS, or every row with --show_ref), contigs in first-seen order
    (the reference's input_variant_dict_id_set_contig, one id per position)"""
    out = OrderedDict()
    for k, v in calls.items():
        if not show_ref and v["filter"] != "PASS":
            continue
        contig = v["ctg"] if ctg_name is None else ctg_name
        out.setdefault(contig, {})[v["pos"]] = v
    return out


# ------------------------------------------------------------------------------------------ the PoN lines the device hands back
def pon_record(line, contigs):
    """What one PoN line (text, line ending included) contributes: nothing for a line whose first character is '#', nor for one that has
    fewer than five tab-separated fields once str.strip() has taken the whitespace off both ends, nor (with `contigs`) for another contig;
    otherwise (CHROM, int(POS), REF, ALT).  int() raises on a POS it rejects - the reference then dies, and so does this step."""
    if line[:1] == "#":
        return None
    fields = line.strip().split("\t", 5)
    if len(fields) < 5 or (contigs is not None and fields[0] not in contigs):
        return None
    return fields[0], int(fields[1]), fields[3], fields[4]


class PonError(Exception):
    pass


def apply_host_lines(lines, sets, ctg_name, require_allele, hit_ids, path):
    """lines: [(line number, bytes)] in file order -> hit_ids (set of (contig, pos)) grows by what the reference's apply_one finds in them.
    A POS that int() rejects raises PonError naming the file and line, where the reference dies with its ValueError."""
    restrict = frozenset(sets) if ctg_name is None else None
    for no, raw in lines:
        line = raw.decode("utf-8", errors="replace")
        try:
            rec = pon_record(line, restrict)
        except ValueError as e:
            raise PonError("{}: line {}: {}".format(path, no, e))
        if rec is None or (ctg_name is not None and rec[0] != ctg_name):
            continue
        chromosome, position, reference, alternate = rec
        contig = chromosome if ctg_name is None else ctg_name
        call = sets.get(contig, {}).get(position)
        if call is None:
            continue
        if not require_allele or (call["ref"] == reference and call["alt"] in alternate.split(",")):
            hit_ids.add((contig, position))


# ------------------------------------------------------------------------------------------ the device scan
class PonScanner:
    """One cto_pon context: the call set goes up once, then one cto_pon_match_file per PoN."""

    def __init__(self, sets):
        from . import _lib
        import numpy as np
        self._lib, self._np = _lib, np
        self.ids = [(c, p) for c, d in sets.items() for p in d]
        names = [c.encode() for c in sets]
        ctg_idx = {c: i for i, c in enumerate(sets)}
        ctg_off = np.cumsum([0] + [len(n) for n in names]).astype(np.int64)
        strs, str_off = [], [0]
        for c, p in self.ids:
            for s in (sets[c][p]["ref"], sets[c][p]["alt"]):
                b = s.encode()
                strs.append(b)
                str_off.append(str_off[-1] + len(b))
        self._keep = [b"".join(names) + b"\0", np.ascontiguousarray(ctg_off), np.array([ctg_idx[c] for c, _ in self.ids], np.int32),
                      np.array([p for _, p in self.ids], np.int64), b"".join(strs) + b"\0", np.array(str_off, np.int64)]
        nb, co, ci, po, sb, so = self._keep
        self.ctx = C.c_void_p()
        _lib.check(_lib.lib.cto_pon_create(C.byref(self.ctx)))
        _lib.check(_lib.lib.cto_pon_set_calls(self.ctx, len(names), nb, co.ctypes.data, len(self.ids), ci.ctypes.data, po.ctypes.data, sb,
                                              so.ctypes.data))

    def match(self, path, only_contig, require_allele):
        """-> (hit ids {(contig, pos)} found on the device, cto_pon_stats, [(line number, bytes)] for the host)"""
        lib, np = self._lib, self._np
        hit = np.zeros(max(1, len(self.ids)), np.uint8)
        st = lib.PonStats()
        lib.check(lib.lib.cto_pon_match_file(self.ctx, path.encode(), None if only_contig is None else only_contig.encode(), int(require_allele),
                                             hit.ctypes.data, C.byref(st), lib.current_stream_ptr()))
        b, o, ln = C.c_void_p(), C.c_void_p(), C.c_void_p()
        n = lib.check(lib.lib.cto_pon_host_lines(self.ctx, C.byref(b), C.byref(o), C.byref(ln)))
        lines = []
        if n:
            off = np.ctypeslib.as_array(C.cast(o, C.POINTER(C.c_int64)), (n + 1,))
            nos = np.ctypeslib.as_array(C.cast(ln, C.POINTER(C.c_int64)), (n,))
            raw = C.string_at(b, int(off[-1]))
            lines = [(int(nos[i]), raw[off[i]:off[i + 1]]) for i in range(n)]
        return {self.ids[i] for i in np.flatnonzero(hit[:len(self.ids)])}, st, lines

    def close(self):
        if self.ctx:
            self._lib.lib.cto_pon_destroy(self.ctx)
            self.ctx = None


def file_md5(path, out):
    h = hashlib.md5()
    with open(path, "rb") as f:
        for chunk in iter(lambda: f.read(1 << 22), b""):
            h.update(chunk)
    out.append(h.hexdigest())


def pon_hits(scanner, path, ctg_name, require_allele, sets, skip_md5, timing=None):
    """one PoN: -> (hit ids, md5 text for the header).  The md5 runs on a host thread while the device scans."""
    md5 = []
    t = None if skip_md5 else threading.Thread(target=file_md5, args=(path, md5))
    if t is not None:
        t.start()
    try:
        hits, st, lines = scanner.match(path, ctg_name, require_allele)
        apply_host_lines(lines, sets, ctg_name, require_allele, hits, path)
    finally:
        if t is not None:
            t.join()
    if timing is not None:
        timing.append(st)
    return hits, ("skipped" if skip_md5 else md5[0])


# ------------------------------------------------------------------------------------------ output
def with_info_lines(header, info):
    """`info` (whole lines) placed right behind the first header line that is the RefCall FILTER line; a header without one is kept as is"""
    lines = header.split("\n")
    if REFCALL_FILTER_LINE not in lines:
        return header
    at = lines.index(REFCALL_FILTER_LINE) + 1
    return "\n".join(lines[:at] + [info.rstrip("\n")] + lines[at:])


def summary_line(ctg, n_input, n_tagged, n_left, pon_fns, pon_hits):
    """the `[INFO] NonSomaticTaggingSummary:` line: key=value pairs joined by ';', the PoNs numbered from 1 and named by file name"""
    pairs = [("ctg", "." if ctg is None else ctg), ("total_input_pass_calls", n_input), ("tagged_non_somatic_union", n_tagged),
             ("remain_pass_calls", n_left), ("num_pon_files", len(pon_fns))]
    for k, (fn, h) in enumerate(zip(pon_fns, pon_hits), 1):
        pairs += [("PoN%d_hits" % k, h), ("PoN%d_file" % k, os.path.basename(str(fn)))]
    return "[INFO] NonSomaticTaggingSummary: " + ";".join("%s=%s" % kv for kv in pairs)


def append_summary_row(path, ctg, counts, pon_fns):
    """One tab-separated row per invocation (contig or '.', then `counts`: input, tagged, remaining, hits of each PoN) appended to the sample's
    summary file under an exclusive flock - the contigs of a run write it concurrently; the file's first writer puts '#PON_PATHS' and the PoN
    paths in front of the rows."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "a", encoding="utf-8") as fh:
        fcntl.flock(fh.fileno(), fcntl.LOCK_EX)                  # released when the file is closed
        if fh.seek(0, os.SEEK_END) == 0:
            fh.write("\t".join(["#PON_PATHS"] + [str(p) for p in pon_fns]) + "\n")
        fh.write("\t".join(str(v) for v in ["." if ctg is None else ctg] + list(counts)) + "\n")


def print_sample_summary(path):
    """The sample's summary line (ctg=ALL) from the rows every contig appended: each count column summed; a PoN column that is missing or not
    a number in some row sums to 0; the PoNs are named from the '#PON_PATHS' line, '.' where it names fewer."""
    if not path or not os.path.isfile(path):
        print("[ERROR] no non-somatic summary file {}".format(path), file=sys.stderr)
        return
    with open(path, encoding="utf-8", errors="replace") as f:
        lines = f.read().split("\n")
    pons = next((ln.split("\t")[1:] for ln in reversed(lines) if ln.startswith("#PON_PATHS")), [])
    rows = [ln.split("\t") for ln in lines if ln.strip() and not ln.startswith("#")]
    if not rows:
        print("[WARNING] no rows in the non-somatic summary file {}".format(path), file=sys.stderr)
        return

    def column(j):
        return sum(int(r[j]) for r in rows)
    try:
        n_input, n_tagged, n_left = column(1), column(2), column(3)
    except (IndexError, ValueError) as e:
        print("[ERROR] non-somatic summary file {}: {}".format(path, e), file=sys.stderr)
        return
    hits = []
    for j in range(4, len(rows[0])):
        try:
            hits.append(column(j))
        except (IndexError, ValueError):
            hits.append(0)
    print(summary_line("ALL", n_input, n_tagged, n_left, (pons + ["."] * len(hits))[:len(hits)], hits))


def contig_order(contigs):
    order = major_contigs_order + list(contigs)
    return sorted(contigs, key=lambda x: order.index(x))


def write_output(fn, header, sets, pon_hits_list, disable_print_nonsomatic_calls):
    """the rows of the reference's writer (:429-461): pon_hits_list[i] = hit ids {(contig, pos)} of PoN i"""
    union = set().union(*pon_hits_list) if pon_hits_list else set()
    with open(fn, "w") as out:
        out.write(header)
        for contig in contig_order(list(sets)):
            for pos in sorted(sets[contig]):
                row = sets[contig][pos]["row"]
                tagged = (contig, pos) in union
                if disable_print_nonsomatic_calls:
                    if not tagged:
                        out.write(row)
                    continue
                columns = row.split("\t")
                if tagged:
                    columns[6] = "NonSomatic"
                    columns[7] = columns[7] + ";" + ";".join("PoN_{}".format(i + 1) for i, h in enumerate(pon_hits_list) if (contig, pos) in h)
                out.write("\t".join(columns))


# ------------------------------------------------------------------------------------------ the step
def nonsomatic_tag(args, timing=None):
    ctg_name = args.ctg_name
    pon_fns = args.panel_of_normals.split(",") if args.panel_of_normals is not None else []
    require_list = args.panel_of_normals_require_allele_matching.split(",") if args.panel_of_normals_require_allele_matching is not None else []
    header, calls = read_pileup_vcf(args.pileup_vcf_fn, ctg_name, args.show_ref, args.input_filter_tag)
    sets = call_sets(calls, ctg_name, args.show_ref)
    total_input = sum(len(d) for d in sets.values())
    print("[INFO] Processing in {}...".format(ctg_name))
    print("[INFO] Processing in {}: total input pass calls: {}".format(ctg_name, total_input))

    pon_hits_list, info = [], ""
    scanner = PonScanner(sets) if pon_fns else None
    try:
        for index, fn in enumerate(pon_fns):
            require_allele = _cli.str2bool(require_list[index])
            hits, md5 = pon_hits(scanner, str(fn), ctg_name, require_allele, sets, args.skip_pon_md5, timing)
            pon_hits_list.append(hits)
            print("[INFO] Processing in {}: tagged by {} PoN: {}".format(ctg_name, str(fn), len(hits)))
            info += ('##INFO=<ID=PoN_{},Number=0,Type=Flag,Description="file={},md5={},allele_matching={},non-somatic variant tagged by panel of '
                     'normals">\n').format(index + 1, str(fn), md5, require_list[index])
    finally:
        if scanner is not None:
            scanner.close()
    union = set().union(*pon_hits_list) if pon_hits_list else set()
    print("[INFO] Processing in {}: tagged by all panel of normals: {}, remained pass calls: {}".format(ctg_name, len(union), total_input - len(union)))
    totals = [len(h) for h in pon_hits_list]
    if args.nonsomatic_summary_aggregate_tsv:
        append_summary_row(args.nonsomatic_summary_aggregate_tsv, ctg_name, [total_input, len(union), total_input - len(union)] + totals, pon_fns)
    if not args.suppress_nonsomatic_tagging_summary or not args.nonsomatic_summary_aggregate_tsv:
        print(summary_line(ctg_name, total_input, len(union), total_input - len(union), pon_fns, totals))
    new_header = with_info_lines(header, info) if info else header
    write_output(args.output_vcf_fn, new_header, sets, pon_hits_list, args.disable_print_nonsomatic_calls)


def build_parser():
    p = argparse.ArgumentParser(description="Non-somatic tagging for pileup data (panel-of-normals scan on the device)")
    p.add_argument("--ctg_name", type=str, default=None)
    p.add_argument("--pileup_vcf_fn", type=str, default=None)
    p.add_argument("--panel_of_normals", type=str, default=None)
    p.add_argument("--panel_of_normals_require_allele_matching", type=str, default=None)
    p.add_argument("--output_vcf_fn", type=str, default=None)
    p.add_argument("--input_filter_tag", type=_cli.str_none, default=None)
    p.add_argument("--show_ref", action="store_true")
    p.add_argument("--disable_print_nonsomatic_calls", action="store_true")
    p.add_argument("--skip_pon_md5", action="store_true")
    p.add_argument("--suppress_nonsomatic_tagging_summary", type=_cli.str2bool, default=True)
    p.add_argument("--nonsomatic_summary_aggregate_tsv", type=_cli.str_none, default=None)
    p.add_argument("--print_sample_nonsomatic_summary_from_tsv", type=_cli.str_none, default=None)
    _cli.add_ignored(p, python="str", threads="int", pypy3="str", parallel="str", samtools="str")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.print_sample_nonsomatic_summary_from_tsv:
        print_sample_summary(args.print_sample_nonsomatic_summary_from_tsv)
        return
    try:
        nonsomatic_tag(args)
    except PonError as e:
        sys.exit("[ERROR] panel of normals: {}".format(e))


if __name__ == "__main__":
    main()
