"""The reference's src/select_hetero_snp_for_phasing.py (run_clairs_to STEP 3): the heterozygous SNP calls of one contig, picked out of
the pileup VCF for the phasing step (phase_tumor here).  Host only: one pass over a VCF.  Pinned to the reference byte for byte - the
output file and the printed line - by tests/golden/select_hetero.json.gz (tests/test_select_hetero.py).

    python -m clairs_to_amd select_hetero_snp_for_phasing --tumor_vcf_fn VCF --output_folder DIR --ctg_name CTG [--var_pct_full F]

Rules kept (src/select_hetero_snp_for_phasing.py:40-103): `|` reads as `/`, so 0/1 and 1/0 both count as heterozygous (0|1 and 1|0 too);
only rows with one REF and one ALT letter are looked at; every such heterozygous row enters the QUAL table, also below --min_qual, which
only keeps it out of the output; the --var_pct_full fraction of lowest QUAL is taken from a stable sort over the table in the order its
positions first came; a later row at a position replaces the earlier one; header rows are copied; plain or gzip input."""
import gzip
import os
import sys
from argparse import SUPPRESS, ArgumentParser


def _open_text(fn):
    with open(fn, "rb") as f:
        gz = f.read(2) == b"\x1f\x8b"
    return gzip.open(fn, "rt") if gz else open(fn)


def select_hetero_snp_for_phasing(args):
    contig = args.ctg_name
    header, rows, quals = [], {}, {}
    not_found = 0
    with _open_text(args.tumor_vcf_fn) as f:
        for row in f:
            row = row.rstrip()
            if row[0] == "#":
                header.append(row + "\n")
                continue
            columns = row.strip().split()
            if contig and contig != columns[0]:
                continue
            if len(columns[3]) != 1 or len(columns[4]) != 1:
                continue
            if columns[9].split(":")[0].replace("|", "/") not in ("0/1", "1/0"):
                continue
            pos, qual = int(columns[1]), float(columns[5])
            quals[pos] = qual                                       # a repeated position keeps its first place in the table
            if qual < args.min_qual:
                not_found += 1
                continue
            rows[pos] = row
    low = set(p for p, _ in sorted(quals.items(), key=lambda x: x[1])[:int(args.var_pct_full * len(quals))])
    keep = {p: r for p, r in rows.items() if p not in low}
    low_qual_count = len(rows) - len(keep)
    pro = round(len(keep) / max(len(quals), 1.0), 4)
    print("[INFO] Total HET SNP calls selected: {}: {}, not found:{}, not match:{}, low_qual_count:{}. Total tumor:{}, pro: {}".format(
        contig, len(keep), not_found, 0, low_qual_count, len(quals), pro))
    os.makedirs(args.output_folder, exist_ok=True)
    with open(os.path.join(args.output_folder, "{}.vcf".format(contig)), "w") as f:
        f.write("".join(header))
        for pos in sorted(keep):
            f.write(keep[pos] + "\n")


def build_parser():
    """every option of the reference's parser (src/select_hetero_snp_for_phasing.py:105-121) at its arity"""
    ap = ArgumentParser(prog="select_hetero_snp_for_phasing", description="Select heterozygous snp candidates for phasing")
    ap.add_argument("--output_folder", type=str, default=None, help="Output folder with all filtered SNP")
    ap.add_argument("--tumor_vcf_fn", type=str, default=None, help="Path of the tumor input vcf file")
    ap.add_argument("--var_pct_full", type=float, default=0.00, help="Default the low quality proportion to be removed in phasing")
    ap.add_argument("--ctg_name", type=str, default=None, help="The name of sequence to be processed, default: %(default)s")
    ap.add_argument("--min_qual", type=float, default=5, help=SUPPRESS)
    return ap


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    ap = build_parser()
    if len(argv) == 0:
        ap.print_help()
        sys.exit(1)
    select_hetero_snp_for_phasing(ap.parse_args(argv))


if __name__ == "__main__":
    main()
