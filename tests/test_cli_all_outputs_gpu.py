"""GPU: the stages of emsar-hip's per-sample run do not lean on each other.  One -M job over two samples (the syn300_se fixture and every
second read of it) with every analysis switched on writes the full set of files; then each analysis runs alone, with only the options it
needs, and must write the same bytes as the job that ran them all.  The CLI solves in deterministic mode, so two runs of one input print
the same bytes (test_cli_gpu.test_two_runs_write_the_same_bytes) and any difference here is a stage reading another stage's leftovers."""
import gzip
import os
import subprocess

import pytest

from emsar_amd import _build
from emsar_amd import hostlib as HL
from tests.conftest import aln_path, get_fixture

pytestmark = pytest.mark.gpu

BASE = {"fpkm", "fraglength_effect"}
GENES = BASE | {"gfpkm"}
PER_SAMPLE = GENES | {"segments", "isoforms", "fit", "gfit", "presence", "profile", "gprofile", "asym", "gasym", "bootstrap", "gbootstrap",
                      "bootq", "gbootq", "saturation", "gsaturation"}
TWO_SAMPLE = {"compare", "gcompare", "ucompare"}                        # sample 1 only
BOOT = ["--bootstrap", "8", "--bootstrap-quantiles", "0.025,0.5,0.975"]
# analysis -> (its options, needs the gene map, the files of every sample, the files of sample 1 alone)
CASES = {
    "solve": ([], False, BASE, set()),
    "segments": (["-g"], False, BASE | {"segments"}, set()),
    "genes": ([], True, GENES, set()),
    "isoforms": (["--isoforms"], True, GENES | {"isoforms"}, set()),
    "fit": (["--fit"], True, GENES | {"fit", "gfit"}, set()),
    "presence": (["--presence"], False, BASE | {"presence"}, set()),
    "profile": (["--profile", "--profile-evals", "30"], True, GENES | {"profile", "gprofile"}, set()),
    "compare": (["--compare"], True, GENES, {"compare", "gcompare"}),
    "compare_usage": (["--compare-usage"], True, GENES, {"ucompare"}),
    "asymptotic": (["--asymptotic"], True, GENES | {"asym", "gasym"}, set()),
    "bootstrap": (["--isoforms"] + BOOT, True, GENES | {"isoforms", "bootstrap", "gbootstrap", "bootq", "gbootq"}, set()),
    "subsample": (["--subsample", "0.5,1", "--subsample-reps", "3"], True, GENES | {"saturation", "gsaturation"}, set()),
}
ALL_ON = ["-g", "--isoforms", "--fit", "--presence", "--profile", "--profile-evals", "30", "--compare", "--compare-usage", "--asymptotic"] + BOOT + \
         ["--subsample", "0.5,1", "--subsample-reps", "3"]


def _files(out):
    """{sample: {extension: bytes}} of a job's output directory"""
    got = {0: {}, 1: {}}
    for name in os.listdir(out):
        prefix, i, ext = name.split(".", 2)
        assert prefix == "out", name
        got[int(i)][ext] = open(os.path.join(out, name), "rb").read()
    return got


@pytest.fixture(scope="module")
def job(tmp_path_factory):
    """the inputs, a runner of the CLI over them, and the files of the job with everything on"""
    _build.build_all()
    tmp = tmp_path_factory.mktemp("all_outputs")
    fx = get_fixture("syn300_se")
    rsh_path = os.path.join(fx.dir, "index.rsh")
    lines = gzip.open(aln_path(fx.dir)[0], "rt").read().splitlines(True)
    names = []
    for l in lines:
        if not names or names[-1] != l.split("\t")[0]:
            names.append(l.split("\t")[0])
    keep = set(names[::2])
    alns = [tmp / "full.bowtie.gz", tmp / "half.bowtie.gz"]
    with gzip.open(alns[0], "wt") as f:
        f.write("".join(lines))
    with gzip.open(alns[1], "wt") as f:
        f.write("".join(l for l in lines if l.split("\t")[0] in keep))
    lst = tmp / "samples.list"
    lst.write_text("".join(str(p) + "\n" for p in alns))
    g2t = tmp / "genes.g2t"
    g2t.write_text("".join("gene%04d\t%s\n" % (t // 3, name) for t, name in enumerate(HL.HostRsh(rsh_path).names)))

    def run(name, extra, genes):
        out = tmp / name
        cmd = [_build.CLI, "-q", "-M", "--gpus", "1", "-i", "20000"] + fx.meta["opts"] + (["--g2t", str(g2t)] if genes else []) + extra
        subprocess.run(cmd + ["-I", rsh_path, str(out), "out", str(lst)], check=True, timeout=300)
        return _files(str(out))

    return run, run("all", ALL_ON, True)


def test_the_job_with_everything_on_writes_every_file(job):
    _, everything = job
    assert len(PER_SAMPLE) == 18
    assert set(everything[0]) == PER_SAMPLE and set(everything[1]) == PER_SAMPLE | TWO_SAMPLE
    assert all(len(b) > 0 for s in everything.values() for b in s.values())


@pytest.mark.parametrize("analysis", list(CASES))
def test_an_analysis_alone_writes_the_same_bytes(job, analysis):
    """.isoforms carries the bootstrap's columns in the job with everything on, so the point estimate alone ("isoforms") is compared by its own
    five columns, as printed; with the bootstrap ("bootstrap") the file is compared byte for byte like every other file"""
    run, everything = job
    extra, genes, per_sample, second = CASES[analysis]
    alone = run(analysis, extra, genes)
    assert set(alone[0]) == per_sample and set(alone[1]) == per_sample | second
    for i in (0, 1):
        for ext, data in alone[i].items():
            if analysis == "isoforms" and ext == "isoforms":
                cut = lambda b: [l.split(b"\t")[:5] for l in b.splitlines()]
                assert cut(data) == cut(everything[i][ext]) and len(cut(data)) > 1, (i, ext)
            else:
                assert data == everything[i][ext], (i, ext)
