"""`python -m clairs_to_amd <submodule> ...` - same dispatch style as the reference's clairs_to.py:84-107 for the
hot-path sub-modules this package replaces and the post-calling steps it mirrors (the short-read chain is complete: realign_variants ->
postfilter_variants -> postprocess_vcf); each takes the argv run_clairs_to builds for its namesake (tests/test_cli_argv.py).
allele_counter takes alleleCounter's own options (the first command of the Verdict step, src/cna_germline_tagging.py:56-71).
get_logr_and_baf and predict_germline_genotypes are steps 2 and 4 of that chain (:92-127): allele counts -> BAF -> germline genotypes;
correct_logr is step 3 (:167-197): the logR corrected for GC content and replication timing, the table the later steps are handed;
aspcf is its segmentation step (:130-140): logR, BAF and genotypes -> segmented logR and BAF; run_ascat (:143-164) turns those into the
tumour's purity, ploidy and copy-number segments; tag_germline_variant (:157-164) is the last step: the exact binomial tests that set
germline-looking PASS calls to LowQual and append the Verdict_* tags.  cna_germline_tagging is that chain's driver as run_clairs_to
starts it: the seven steps, in this process.  cal_af_distribution is the reference's src/cal_af_distribution.py, the AF half of its
compare_vcf step: per truth variant the depth, ALT count and haplotype counts the tumour BAM shows, one pass over the BAM.  compare_vcf is the command the reference's quick demos end with (src/compare_vcf.py): the
calls against a truth set -> precision, recall and F1, the classification and the cut-off sweeps on the GPU.
select_hetero_snp_for_phasing and phase_tumor are the long-read steps between STEP 3 and STEP 4 of run_clairs_to: the heterozygous SNP
calls of a contig, then their phase and the haplotagged BAM (HP, PS) that haplotype_filtering reads - instead of longphase / whatshap.
gen_contaminated_bam is the reference's src/gen_contaminated_bam.py: a tumour BAM of a chosen purity from a tumour and a normal BAM -
coverage, subsample and merge on the GPU instead of mosdepth and samtools.
add_back_missing_variants_in_genotyping ends a --genotyping_mode_vcf_fn / --hybrid_mode_vcf_fn run: the list's uncalled sites go back into
the VCF as ./. rows with the depth and A/C/G/T counts of the _hybrid_info files - lines, keys, one sort and the rows' text on the GPU.
    usage: python -m clairs_to_amd compare_vcf --truth_vcf_fn TRUTH --input_vcf_fn CALLS [--bed_fn BED] [--ctg_name CTG] [--output_dir DIR]"""
import importlib
import sys

SUBMODULES = ("extract_candidates_calling", "concat_files", "create_tensor_pileup_calling", "predict", "call_variants", "pileup_call", "call_chunks",
              "sort_vcf", "postprocess_vcf", "haplotype_filtering", "realign_reads", "realign_variants",
              "nonsomatic_tagging", "postfilter_variants", "allele_counter", "get_logr_and_baf", "predict_germline_genotypes", "aspcf", "run_ascat",
              "correct_logr", "tag_germline_variant", "cna_germline_tagging", "cal_af_distribution", "compare_vcf",
              "select_hetero_snp_for_phasing", "phase_tumor", "gen_contaminated_bam", "add_back_missing_variants_in_genotyping")


def dispatch(name, argv):
    """Run sub-module `name` on `argv` (a list, without the program and sub-module names) in this process."""
    if name in ("sort_vcf", "postprocess_vcf"):          # the host-side tail lives in one module
        mod = importlib.import_module("clairs_to_amd.postprocess_vcf")
        return getattr(mod, name + "_main")(argv)
    return importlib.import_module("clairs_to_amd." + name).main(argv)


def main():
    if len(sys.argv) < 2 or sys.argv[1] not in SUBMODULES:
        sys.exit("usage: python -m clairs_to_amd {%s} [options]" % "|".join(SUBMODULES))
    name = sys.argv.pop(1)
    dispatch(name, sys.argv[1:])


if __name__ == "__main__":
    main()
