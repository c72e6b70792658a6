"""The reference's src/add_back_missing_variants_in_genotyping.py: the command that ends a --genotyping_mode_vcf_fn or --hybrid_mode_vcf_fn
run.  Every site of the user's list that was not called goes back into the VCF as a `./.` row with the tumour's depth and A/C/G/T counts
from the `<ctg>.<chunk>_hybrid_info` files that extract_candidates_calling and call_chunks wrote.

    python -m clairs_to_amd add_back_missing_variants_in_genotyping --call_fn CALLS.vcf --output_fn OUT.vcf
        (--genotyping_mode_vcf_fn LIST | --hybrid_mode_vcf_fn LIST) [--candidates_folder DIR] [--switch_genotype True]
        [--where device|host] [--threads N]

Text in, text out: the files' bytes go to one cto_add_back call (csrc/addback.hip: the eleven rules, the kernels, the host path), which
finds the lines, parses the keys, sorts the records of the three sources once and writes the rows.  What the call will not decide exactly
it reports and this module's own restatement of the rules (`restate`, plain Python, dicts) writes the output instead:
  * `non_ascii`: a text with '\\r' or a byte >= 0x80 - universal newlines and Unicode whitespace and digits are Python's to read;
  * `undecided`: a POS or a count that is not 1-18 plain ASCII digits yet holds a digit ('+5', '1_0', a 19-digit POS), or a POS of 2^42 or more.
Both are counted in the `stats` dict of add_back(); neither is silent.

Where the reference has no rule this module has one: contigs outside the reference's major list follow the major ones in order of first
appearance (calls, then list; the reference iterates a set there); the `hybrid_info` files are read in sorted-name order (os.listdir order
there).  A line of the calls or the list without two tokens, a blank one included, crashes the reference with an IndexError; here the run
ends with an error that names the file and the line."""
import argparse
import ctypes as C
import gzip
import os
import shutil
import sys

from ._cli import str2bool, str_none
from .postprocess_vcf import compress_index_vcf

major_contigs_order = ["chr" + str(a) for a in list(range(1, 23)) + ["X", "Y"]] + [str(a) for a in list(range(1, 23)) + ["X", "Y"]]
GENOTYPING, HYBRID = 0, 1
FORMAT = "GT:DP:AU:CU:GU:TU"


def _default_where():
    import torch
    return "device" if torch.cuda.is_available() else "host"


class BadLine(ValueError):
    """a line of the calls or the list without two tokens: (source 1 calls / 2 list, 1-based line)"""

    def __init__(self, source, line):
        ValueError.__init__(self, "line %d of the %s has no CHROM and POS" % (line, ("calls", "list")[source - 1]))
        self.source, self.line = source, line


# ------------------------------------------------------------------------------------------------ files
def read_text(path):
    """the inflated bytes of a plain or gzip file (`gzip -fdc`); b"" for a missing one, as the reference reads no record from it"""
    if path is None or not os.path.exists(path):
        return b""
    with open(path, "rb") as f:
        raw = f.read()
    return gzip.decompress(raw) if raw[:2] == b"\x1f\x8b" else raw


def read_info_folder(folder):
    """every file of the folder whose name ends in hybrid_info, in sorted-name order, back to back; each file's last line is closed so that
    no line runs on into the next file"""
    if folder is None or not os.path.exists(folder):
        return b""
    parts = []
    for name in sorted(os.listdir(folder)):
        if name.endswith("hybrid_info"):
            with open(os.path.join(folder, name), "rb") as f:
                text = f.read()
            parts.append(text if not text or text.endswith(b"\n") else text + b"\n")
    return b"".join(parts)


# ------------------------------------------------------------------------------------------------ the restatement
def read_records(text, source):
    """(header, {(CHROM, POS): row}): '#' rows in file order; of the rows of one key the last, at the key's first place"""
    header, rows = [], {}
    s = text.decode("utf-8", "surrogateescape").replace("\r\n", "\n").replace("\r", "\n") if text else ""
    parts = s.split("\n")
    n = len(parts)
    for i, body in enumerate(parts):
        last = i == n - 1
        if last and body == "":
            break
        row = body if last else body + "\n"
        columns = row.strip().split()
        if not columns or (columns[0][0] != "#" and len(columns) < 2):
            raise BadLine(source, i + 1)
        if columns[0][0] == "#":
            header.append(row)
            continue
        rows[(columns[0], int(columns[1]))] = row
    return "".join(header), rows


def read_info(text):
    """{(contig, POS): (ref_base, depth-seqs field)} of the hybrid_info rows with four columns or more; the last row of a key counts"""
    info = {}
    s = text.decode("utf-8", "surrogateescape").replace("\r\n", "\n").replace("\r", "\n") if text else ""
    for body in s.split("\n"):
        columns = body.split("\t")
        if len(columns) < 4:
            continue
        info[(columns[0], int(columns[1]))] = (columns[2], columns[3])
    return info


def alt_counts(field):
    """DP, AU, CU, GU, TU of "<depth>-<key> <n> <key> <n> ..."; five zeros for anything else"""
    if not field:
        return 0, 0, 0, 0, 0
    try:
        depth, seqs = field.split("-")
        items = seqs.split(" ")
        numbers = [int(x) for x in items[1::2]]
        seen = dict(zip(items[0::2], numbers))
        return (int(depth),) + tuple(seen.get(b, 0) for b in "ACGT")
    except Exception:
        return 0, 0, 0, 0, 0


def rewrite_row(row, ref_base=None, field=None):
    """an uncalled list row as a ./. row"""
    c = row.rstrip().split("\t")
    c += ["."] * (10 - len(c))
    c[3] = c[3][:1] or "."
    if ref_base and ref_base != c[3]:
        c[3] = ref_base
    c[4:10] = [".", ".", ".", ".", FORMAT, "./.:%d:%d:%d:%d:%d" % alt_counts(field)]
    return "\t".join(c) + "\n"


def contig_order(names):
    """the major contigs in the reference's order, then the others as they first appear in `names`"""
    seen = list(dict.fromkeys(names))
    major = {c: k for k, c in enumerate(major_contigs_order)}
    return sorted(seen, key=lambda c: (major.get(c, len(major)), seen.index(c) if c not in major else 0))


def restate(calls, listed, info, mode, switch_genotype):
    """(output bytes, (list keys, call keys, added)) by the reference's rules on the three texts, in plain Python"""
    header, called = read_records(calls, 1)
    _, wanted = read_records(listed, 2)
    infos = read_info(info) if switch_genotype else {}
    rows, added = {}, 0
    if mode == HYBRID:
        rows.update(called)
    for key, row in wanted.items():
        if key in called:
            rows[key] = called[key]
            continue
        added += 1
        rows[key] = rewrite_row(row, *infos.get(key, (None, None))) if switch_genotype else row
    order = {c: k for k, c in enumerate(contig_order([k[0] for k in called] + [k[0] for k in wanted]))}
    body = "".join(rows[k] for k in sorted(rows, key=lambda k: (order[k[0]], k[1])))
    return (header + body).encode("utf-8", "surrogateescape"), (len(wanted), len(called), added)


# ------------------------------------------------------------------------------------------------ the C call
def sort_u64(keys, payload, where="device"):
    """cto_sort_u64: (keys, payload) sorted by key, equal keys in input order; numpy uint64 / uint32 arrays in, new arrays out"""
    import numpy as np
    from ._lib import check, current_stream_ptr, lib
    if where not in ("device", "host"):
        raise ValueError("where must be 'device' or 'host'")
    k = np.array(keys, dtype=np.uint64, copy=True)
    p = np.array(payload, dtype=np.uint32, copy=True)
    if k.shape != p.shape or k.ndim != 1:
        raise ValueError("keys and payload are two vectors of one length")
    stream = C.c_void_p(current_stream_ptr()) if where == "device" else None
    check(lib.cto_sort_u64(k.ctypes.data, p.ctypes.data, len(k), 0 if where == "device" else 1, stream))
    return k, p


def add_back(calls, listed, info, mode, switch_genotype=True, where="device", host_threads=0, stats=None):
    """(output bytes, (list keys, call keys, added)) of cto_add_back on the three texts (bytes).  where: "device" (HIP kernels on the current
    stream) or "host".  stats: a dict that receives the call's cto_add_back_stats and `restated`: why the Python restatement wrote the
    output instead (None, "non_ascii" or "undecided").  A line without CHROM and POS raises BadLine."""
    from ._lib import AddBackStats, check, current_stream_ptr, lib
    if where not in ("device", "host"):
        raise ValueError("where must be 'device' or 'host'")
    if mode not in (GENOTYPING, HYBRID):
        raise ValueError("mode is GENOTYPING or HYBRID")
    st = AddBackStats()
    counts = (C.c_int64 * 3)()
    stream = C.c_void_p(current_stream_ptr()) if where == "device" else None
    cap = len(calls) + len(listed) + 160 * (listed.count(b"\n") + 1) + (len(info) if switch_genotype else 0)
    while True:
        out = C.create_string_buffer(max(cap, 1))
        n = check(int(lib.cto_add_back(calls, len(calls), listed, len(listed), info, len(info), mode, int(bool(switch_genotype)),
                                       0 if where == "device" else 1, host_threads, stream, out, cap, counts, C.byref(st))))
        if n <= cap:
            break
        cap = n
    why = "non_ascii" if st.non_ascii else "undecided" if st.undecided else None
    if stats is not None:
        stats.update(n_lines=list(st.n_lines), n_rows=st.n_rows, undecided=st.undecided, non_ascii=st.non_ascii, bad_source=st.bad_source,
                     bad_line=st.bad_line, host_path=st.host_path, kernel_ms=st.kernel_ms, restated=why)
    if st.bad_source:
        raise BadLine(int(st.bad_source), int(st.bad_line))
    if why:
        return restate(calls, listed, info, mode, switch_genotype)
    return C.string_at(out, n), tuple(counts)


# ------------------------------------------------------------------------------------------------ the command
def build_parser():
    ap = argparse.ArgumentParser(description="Genotype VCF in postprocessing (mirror of src/add_back_missing_variants_in_genotyping.py)")
    ap.add_argument("--genotyping_mode_vcf_fn", type=str_none, default=None, help="Candidate sites VCF file input for genotyping")
    ap.add_argument("--hybrid_mode_vcf_fn", type=str_none, default=None,
                    help="Variants that passed the threshold and additional VCF candidates will both be subjected to variant calling")
    ap.add_argument("--candidates_folder", type=str, default=None, help="Candidate folder with the *hybrid_info files")
    ap.add_argument("--call_fn", type=str, default=None, help="Somatic VCF input")
    ap.add_argument("--output_fn", type=str, default=None, help="Output vcf file name")
    ap.add_argument("--switch_genotype", type=str2bool, default=True, help="Switch missed variant genotype to ./.")
    ap.add_argument("--where", choices=("device", "host"), default=None, help="device: the HIP kernels (default with a GPU); host: the library's host path")
    ap.add_argument("--threads", type=int, default=0, help="threads of the host path (0: 16)")
    return ap


def genotype_vcf(args, stats=None):
    if args.genotyping_mode_vcf_fn is None and args.hybrid_mode_vcf_fn is None:
        sys.exit("[ERROR] Both VCF {} and additional VCF is None, exit!".format(args.genotyping_mode_vcf_fn, args.hybrid_mode_vcf_fn))
    genotyping = args.genotyping_mode_vcf_fn is not None
    list_fn = args.genotyping_mode_vcf_fn if genotyping else args.hybrid_mode_vcf_fn
    with open(args.output_fn, "wb") as output:                     # opened first, as the reference does: a failed run leaves it empty
        try:
            shutil.copyfile(args.call_fn, args.call_fn + ".bak")       # `cp call_fn call_fn.bak`, outcome unchecked
        except (OSError, TypeError):
            pass
        calls, listed = read_text(args.call_fn), read_text(list_fn)
        info = read_info_folder(args.candidates_folder)
        try:
            text, counts = add_back(calls, listed, info, GENOTYPING if genotyping else HYBRID, args.switch_genotype,
                                    where=args.where or _default_where(), host_threads=args.threads, stats=stats)
        except BadLine as e:
            sys.exit("add_back_missing_variants_in_genotyping: line {} of {} has no CHROM and POS".format(e.line, args.call_fn if e.source == 1 else list_fn))
        output.write(text)
    print("[INFO] Total {}variants for genotyping: {}, total tumor-only somatic variant calls: {}, added {} variants into output VCF".format(
        "" if genotyping else "additional ", *counts))
    compress_index_vcf(args.output_fn)


def main(argv=None):
    genotype_vcf(build_parser().parse_args(argv))


if __name__ == "__main__":
    main()
