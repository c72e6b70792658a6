"""What the add_back tests share: the fixture's files on disk, a seeded generator of random cases, and a naive restatement of the command
(dicts and Python's own int / split) that owes nothing to the module's."""
import gzip
import os
import random
import re

from conftest import load_json_gz

MAJOR = ["chr" + str(a) for a in list(range(1, 23)) + ["X", "Y"]] + [str(a) for a in list(range(1, 23)) + ["X", "Y"]]
_cache = {}


def golden():
    if "g" not in _cache:
        _cache["g"] = load_json_gz("add_back.json.gz")
    return _cache["g"]


def write_inputs(d, texts):
    """the files the fixture's argv lists name, in directory d (what gen_add_back.write_inputs wrote for the reference)"""
    os.makedirs(os.path.join(d, "cand"))
    for name, key in (("calls.vcf", "calls"), ("calls_nonl.vcf", "calls_nonl"), ("list.vcf", "list"), ("list_nonl.vcf", "list_nonl"),
                      ("list_called.vcf", "list_called"), ("list_header.vcf", "list_header")):
        with open(os.path.join(d, name), "w") as f:
            f.write(texts[key])
    for name, key in (("calls.vcf.gz", "calls"), ("list.vcf.gz", "list")):
        with gzip.open(os.path.join(d, name), "wt") as f:
            f.write(texts[key])
    for name, text in texts["info"].items():
        with open(os.path.join(d, "cand", name), "w") as f:
            f.write(text)
    with open(os.path.join(d, "cand", "chr1.1_snv"), "w") as f:
        f.write("chr1\t21\tA\t1-A 1\n")


def config_argv(cf, d, where=None):
    return [a.replace("@D@", str(d)) for a in cf["argv"]] + (["--where", where] if where else [])


def config_texts(cf, texts):
    """(calls, list, info, mode, switch_genotype) of a fixture configuration as the C call takes them"""
    ns = cf["namespace"]
    keys = {"calls.vcf": "calls", "calls.vcf.gz": "calls", "calls_nonl.vcf": "calls_nonl", "list.vcf": "list", "list.vcf.gz": "list",
            "list_nonl.vcf": "list_nonl", "list_called.vcf": "list_called", "list_header.vcf": "list_header"}
    text_of = lambda p: texts[keys[os.path.basename(p)]] if p and os.path.basename(p) in keys else ""
    geno = ns["genotyping_mode_vcf_fn"] is not None
    lst = ns["genotyping_mode_vcf_fn"] if geno else ns["hybrid_mode_vcf_fn"]
    folder = ns["candidates_folder"]
    info = "".join(texts["info"][k] for k in sorted(texts["info"])) if folder and folder.endswith("/cand") else ""
    return text_of(ns["call_fn"]).encode(), text_of(lst).encode(), info.encode(), 0 if geno else 1, ns["switch_genotype"]


# ------------------------------------------------------------------------------------------------ the naive restatement
def naive_counts(field):
    if field is None or field == "":
        return [0] * 5
    try:
        depth, seqs = field.split("-")
        seqs = seqs.split(" ")
        d = dict(zip(seqs[::2], [int(x) for x in seqs[1::2]]))
        return [int(depth)] + [d.get(b, 0) for b in "ACGT"]
    except Exception:
        return [0] * 5


def naive_info(info):
    out = {}
    for row in info.decode().split("\n"):
        c = row.split("\t")
        if len(c) >= 4:
            out[(c[0], int(c[1]))] = (c[2], c[3])
    return out


def naive(calls, listed, info, mode, switch_genotype):
    """(bytes, counts) for ASCII texts without '\\r': one dict per file, one sorted() at the end"""
    def rows_of(text):
        head, rows = "", {}
        for row in re.findall(r"[^\n]*\n|[^\n]+$", text.decode()):
            tok = row.split()
            if tok[0].startswith("#"):
                head += row
            else:
                rows[(tok[0], int(tok[1]))] = row
        return head, rows
    head, called = rows_of(calls)
    _, wanted = rows_of(listed)
    infos = naive_info(info)
    out = dict(called) if mode == 1 else {}
    added = 0
    for k, row in wanted.items():
        if k in called:
            out[k] = called[k]
            continue
        added += 1
        if switch_genotype:
            c = row.rstrip().split("\t")
            c += ["."] * max(0, 10 - len(c))
            ref = c[3][0] if c[3] else "."
            rb = infos.get(k, ("", None))[0]
            c[3:10] = [rb if rb not in ("", ref) else ref, ".", ".", ".", ".", "GT:DP:AU:CU:GU:TU",
                       "./.:" + ":".join(str(v) for v in naive_counts(infos.get(k, ("", None))[1]))]
            row = "\t".join(c) + "\n"
        out[k] = row
    contigs = []
    for k in list(called) + list(wanted):
        if k[0] not in contigs:
            contigs.append(k[0])
    rank = {c: (MAJOR.index(c) if c in MAJOR else len(MAJOR) + [x for x in contigs if x not in MAJOR].index(c)) for c in contigs}
    body = "".join(out[k] for k in sorted(out, key=lambda k: (rank[k[0]], k[1])))
    return (head + body).encode(), (len(wanted), len(called), added)


# ------------------------------------------------------------------------------------------------ random cases
def random_case(seed, n_list, call_share=0.3, contigs=("chr2", "chr10", "3", "chrUn_A", "chrUn_B", "chrX"), span=None, repeat=0):
    """(calls, list, info) texts: n_list list rows over `contigs` at random positions (repeats happen), calls for a share of them and some of
    their own, an info row for most list rows; unsorted throughout.  repeat: that many more copies of one list key, with changing columns."""
    rng = random.Random(seed)
    span = span or max(50, n_list // 2)
    head = "##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS\n"
    calls, listed, info = [], [], []
    for i in range(n_list):
        c, p = rng.choice(contigs), rng.randrange(1, span)
        cols = [c, str(p), ".", rng.choice(("A", "C", "GT", "")), rng.choice("ACGT"), "3", "PASS", "X=%d" % i, "GT", "0/1", "e%d" % i]
        listed.append("\t".join(cols[:rng.choice((2, 4, 5, 8, 10, 11))]) + "\n")
        if rng.random() < call_share:
            calls.append("%s\t%d\t.\tA\tC\t%d\tPASS\t.\tGT\t0/1\n" % (c, p, i))
        if rng.random() < 0.1:
            calls.append("%s\t%d\t.\tA\tC\t%d\tLowQual\t.\tGT\t0/1\n" % (c, p + span, i))
        if rng.random() < 0.8:
            field = rng.choice(("%d-A %d C %d" % (rng.randrange(99), rng.randrange(50), rng.randrange(10 ** 9)), "%d-" % i, "12-T 4 -AG 1", "",
                                "5-G 1 G 2 N 3", "z-A 1", "8-A", "8-A  2", "%d-C %d T" % (i, i)))
            info.append("%s\t%d\t%s\t%s\n" % (c, p, rng.choice(("A", "C", "", "GT")), field))
    for k in range(repeat):
        listed.append("%s\t%d\t.\tA\tC\t%d\n" % (contigs[0], span + 7, k))
    rng.shuffle(info)
    return (head + "".join(calls)).encode(), (head + "".join(listed)).encode(), "".join(info).encode()
