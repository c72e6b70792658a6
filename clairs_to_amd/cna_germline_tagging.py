"""The Verdict step as run_clairs_to starts it (src/cna_germline_tagging.py of the reference): the seven commands of its chain, here the
seven mirrors of this package run one after another in this process through the dispatch of `python -m clairs_to_amd`, in the
reference's order and with its file names.

    python -m clairs_to_amd cna_germline_tagging --tumor_bam_fn BAM --input_vcf_fn VCF --output_fn VCF --output_dir DIR --contig_fn F
           --cna_resource_dir DIR [--tumor_sample_name tumor] [--threads N] [--is_indel] [every other option of the reference's parser]

  1 allele_counter               per contig of --contig_fn among chr1..22, X: <resource>/loci_files/G1000_loci_hg38_<contig>.txt ->
                                 <output_dir>/<sample>_AlleleCount_<contig>.txt, with -m 20 -q 20 -f 0 -F 2316 --dense-snps
  2 get_logr_and_baf             -> <sample>_Tumor_LogR.txt, <sample>_Tumor_BAF.txt
  3 correct_logr                 -> <sample>_Tumor_LogR_Correction.txt
  4 predict_germline_genotypes   -> <sample>_Tumor_GG.txt
  5 aspcf                        -> <sample>_Tumor_LogR_PCFed.txt, <sample>_Tumor_BAF_PCFed.txt
  6 run_ascat                    -> <sample>_Tumor_Purity_Ploidy.txt, <sample>_Tumor_CNA.txt
  7 tag_germline_variant         --input_vcf_fn -> --output_fn

The reference runs step 1 under GNU parallel, one alleleCounter per contig, and steps 2-7 as `python <verdict>/<step>.py ...`; the
argument lists are the same here, step 1 in the per-contig mode of allele_counter.  --parallel, --python, --allele_counter, --verdict,
--normal_bam_fn, --tumor_purity and --platform are accepted and not used.  --is_indel runs the tagging alone.  The output folder is
made when it is not there.  A step that fails prints the reference's line, which shows the command as the reference would have run it
(for the whole chain as the one-element tuple its loop holds), and the exit status is 1."""
import argparse
import os
import shlex
import sys

from .allele_counter import MAJOR_CONTIGS

STEPS = ("allele_counter", "get_logr_and_baf", "correct_logr", "predict_germline_genotypes", "aspcf", "run_ascat", "tag_germline_variant")


def get_contigs(contig_fn):
    with open(contig_fn) as f:
        return [c.strip() for c in f if c.strip() in MAJOR_CONTIGS]


def commands(a):
    """the seven command lines of the reference for these options, in its order"""
    out, name, res, py = a.output_dir, a.tumor_sample_name, a.cna_resource_dir, "%s %s/" % (a.python, a.verdict)
    stem = "%s/%s_Tumor_" % (out, name)
    counter = ('%s -j%s LD_LIBRARY_PATH="$LD_LIBRARY_PATH:%s/lib" %s/bin/alleleCounter -b %s -l %s/loci_files/G1000_loci_hg38_{1}.txt '
               '-o %s/%s_AlleleCount_{1}.txt -m 20 -q 20 -f 0 -F 2316 --dense-snps  ::: %s'
               % (a.parallel, a.threads, a.allele_counter, a.allele_counter, a.tumor_bam_fn, res, out, name, ' '.join(get_contigs(a.contig_fn))))
    logr_baf = (py + "get_logr_and_baf.py --tumor_allele_counts_file_prefix %s/%s_AlleleCount_ --alleles_file_prefix %s/allele_files/G1000_alleles_hg38_ "
                "--tumor_logr_output_file %sLogR.txt --tumor_baf_output_file %sBAF.txt --sample_name %s --contig_fn %s" % (out, name, res, stem, stem, name, a.contig_fn))
    correct = (py + "correct_logr.py --tumor_logr_file %sLogR.txt --gc_content_file %s/GC_G1000_hg38.txt --replication_timing_file %s/RT_G1000_hg38.txt "
               "--tumor_logr_correction_output_file %sLogR_Correction.txt --sample_name %s" % (stem, res, res, stem, name))
    genotypes = (py + "predict_germline_genotypes.py --tumor_logr_file %sLogR_Correction.txt --tumor_baf_file %sBAF.txt --germline_genotypes_output_file %sGG.txt "
                 "--maxHomozygous 0.02 --proportionHetero 0.30 --proportionHomo 0.65 --proportionOpen 0.03 --segmentLength 100 --sample_name %s"
                 % (stem, stem, stem, name))
    tables = "--tumor_logr_file %sLogR_Correction.txt --tumor_baf_file %sBAF.txt --germline_genotypes_file %sGG.txt " % (stem, stem, stem)
    aspcf = (py + "aspcf.py " + tables + "--tumor_logr_pcfed_output_file %sLogR_PCFed.txt --tumor_baf_pcfed_output_file %sBAF_PCFed.txt --penalty 1000 "
             "--sample_name %s" % (stem, stem, name))
    results = "--tumor_purity_ploidy_output_file %sPurity_Ploidy.txt --tumor_cna_output_file %sCNA.txt" % (stem, stem)
    ascat = (py + "run_ascat.py " + tables + "--tumor_logr_segmented_file %sLogR_PCFed.txt --tumor_baf_segmented_file %sBAF_PCFed.txt " % (stem, stem)
             + results + " --sample_name %s" % name)
    tag = py + "tag_germline_variant.py --input_vcf_fn %s --output_fn %s " % (a.input_vcf_fn, a.output_fn) + results
    return [counter, logr_baf, correct, genotypes, aspcf, ascat, tag]


def step_argv(a, step, command):
    """what the mirror of step `step` (0-based) is handed"""
    if step == 0:
        return ["-b", a.tumor_bam_fn, "--contig_fn", a.contig_fn, "--loci_prefix", "%s/loci_files/G1000_loci_hg38_" % a.cna_resource_dir,
                "--output_prefix", "%s/%s_AlleleCount_" % (a.output_dir, a.tumor_sample_name), "-m", "20", "-q", "20", "-f", "0", "-F", "2316", "--dense-snps"]
    return shlex.split(command)[2:]                             # behind the interpreter and the script


def run_step(name, argv):
    """True when the step came to its end"""
    from .__main__ import dispatch
    try:
        dispatch(name, argv)
    except SystemExit as e:
        if e.code not in (None, 0):
            if not isinstance(e.code, int):
                sys.stderr.write(str(e.code) + "\n")
            return False
    except Exception as e:
        sys.stderr.write("%s: %s: %s\n" % (name, type(e).__name__, e))
        return False
    return True


def get_cna_purity(a):
    a.verdict = a.verdict if a.verdict else os.path.dirname(os.path.abspath(__file__))
    if a.output_dir is not None and not os.path.exists(a.output_dir):
        os.makedirs(a.output_dir, exist_ok=True)
    lines = commands(a)
    if not a.is_indel:
        for i, command in enumerate(lines):
            if not run_step(STEPS[i], step_argv(a, i, command)):
                sys.stderr.write("ERROR in STEP {}, THE FOLLOWING COMMAND FAILED: {}\n".format(i + 1, (command,)))
                sys.exit(1)
    elif not run_step(STEPS[6], step_argv(a, 6, lines[6])):
        sys.stderr.write("ERROR in STEP {}, THE FOLLOWING COMMAND FAILED: {}\n".format(1, lines[6]))
        sys.exit(1)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="cna_germline_tagging", description="the Verdict chain, seven steps in this process")
    ap.add_argument('--platform', type=str, default="ont", help="accepted, unused")
    ap.add_argument('--normal_bam_fn', type=str, default=None, help="accepted, unused")
    ap.add_argument('--tumor_bam_fn', type=str, default=None, help="the tumour BAM, with its .bai")
    ap.add_argument('--input_vcf_fn', type=str, default=None, help="the calls to tag")
    ap.add_argument('--tumor_purity', type=float, default=None, help="accepted, unused")
    ap.add_argument('--output_dir', type=str, default=None, help="where the chain's tables go; made when absent")
    ap.add_argument('--output_fn', type=str, default=None, help="the tagged VCF")
    ap.add_argument('--python', type=str, default='python3', help="accepted; the steps run in this process")
    ap.add_argument('--parallel', type=str, default='parallel', help="accepted; the contigs are counted in this process")
    ap.add_argument('--contig_fn', type=str, default=None, help="file of contig names; those among chr1..22, X are used")
    ap.add_argument('--tumor_sample_name', type=str, default='tumor', help="prefix of the chain's file names")
    ap.add_argument('--normal_sample_name', type=str, default='normal', help="accepted, unused")
    ap.add_argument('--allele_counter', type=str, default=None, help="accepted; allele_counter of this package counts")
    ap.add_argument('--cna_resource_dir', type=str, default=None, help="folder with loci_files/, allele_files/, GC_G1000_hg38.txt and RT_G1000_hg38.txt")
    ap.add_argument('--threads', type=int, default=None, help="accepted; it only shows in the command line an error prints")
    ap.add_argument('--verdict', type=str, default=None, help="accepted; the steps are this package's")
    ap.add_argument('--is_indel', action='store_true', help="run the tagging alone")
    get_cna_purity(ap.parse_args(argv))
    return 0


if __name__ == "__main__":
    main(sys.argv[1:])
