"""CPU: every message emsar-hip's option handling can print -- the range messages of the option switch, the "wants a" messages of the
count, seed, fraction-list and device-list parsers, the cross-option checks between the switch and the index read, and the checks on the
sample list -- with its exit status, whether the usage text follows, and which message wins when an argument list trips two checks.  No
device is visible and the index does not exist: every case must end before any input is opened and before the output directory is made."""
import os
import subprocess

import pytest

from emsar_amd import _build

BOOT = "--bootstrap wants a number of replicates (0 .. 1000000)."
BSEED = "--bootstrap-seed wants a non-negative integer."
REPS = "--subsample-reps wants a number of replicates (1 .. 1000000)."
SSEED = "--subsample-seed wants a non-negative integer."
SUB = "--subsample wants a comma-separated list of 1 to 64 fractions in (0, 1]."
BQ = "--bootstrap-quantiles wants a comma-separated list of 1 to 64 probabilities in [0, 1]."
DEV = "--devices wants a comma-separated list of device ids."
BQ_NEEDS = "--bootstrap-quantiles needs --bootstrap B with 1 <= B <= 4096 replicates."
ISO_NEEDS = "--isoforms needs --g2t FILE."
CUT_NEEDS = "--boundary-cut needs --asymptotic."
CUT_RANGE = "--boundary-cut must be >= 0."
PRES_NEEDS = "--presence-list needs --presence."
PROF_NEEDS = "--profile-list, --profile-level and --profile-evals need --profile."
LEVEL_RANGE = "--profile-level must lie in (0, 1)."
RATIO_NEEDS = "--compare-ratio needs --compare."
LIST_NEEDS = "--compare-list needs --compare or --compare-usage."
USAGE_G2T = "--compare-usage needs --g2t FILE."
RATIO_RANGE = "--compare-ratio must be positive."
CMP_M = "--compare needs -M and at least two samples."
UCMP_M = "--compare-usage needs -M and at least two samples."
G2T = ["--g2t", "none.g2t"]

# (arguments, the whole of stderr up to the usage text, whether the usage text follows)
SWITCH = [
    (["-n", "0"], "option -n must be a natural number.", False),
    (["-n", "-3"], "option -n must be a natural number.", False),
    (["-n", "x"], "option -n must be a natural number.", False),
    (["-e", "0"], "option -e must be positive.", False),
    (["-e", "-1e-3"], "option -e must be positive.", False),
    (["-i", "0"], "option -i must be positive.", False),
    (["-i", "x"], "option -i must be positive.", False),
    (["--count-floor", "-1"], "--count-floor must be >= 0.", False),
    (["--profile-evals", "0"], "--profile-evals must be positive.", False),
    (["--profile-evals", "-2"], "--profile-evals must be positive.", False),
    (["--profile", "--profile-evals", "x"], "--profile-evals must be positive.", False),
]
COUNTS = [(["--bootstrap", v], BOOT, False) for v in ("", "x", "3x", " ", "-1", "1000001", "99999999999999999999")] + \
         [(["--subsample-reps", v], REPS, False) for v in ("", "x", "3x", "0", "-1", "1000001", "99999999999999999999")]
SEEDS = [([opt, v], msg, False) for opt, msg in (("--bootstrap-seed", BSEED), ("--subsample-seed", SSEED))
         for v in ("", "x", "7x", "-1", "99999999999999999999")]
LIST65 = ",".join(["0.5"] * 65)
LISTS = [(["--subsample", v], SUB, False) for v in ("", "x", "0.5;1", "0.5,", ",0.5", "0.5,,1", "0", "-0.5", "1.5", "nan", "inf", "1e999", LIST65)] + \
        [(["--bootstrap", "8", "--bootstrap-quantiles", v], BQ, False)
         for v in ("", "x", "0.5;1", "0.5,", ",0.5", "0.5,,1", "-0.1", "1.5", "nan", "inf", "1e999", LIST65)]
DEVICES = [(["--devices", v], DEV, False) for v in ("", "x", "0,x", "0x", "0,,1", ",0", "-1", "0,-1", "1024", "99999999999999999999")]
CROSS = [
    (["--bootstrap-quantiles", "0.5"], BQ_NEEDS, False),
    (["--bootstrap", "0", "--bootstrap-quantiles", "0.5"], BQ_NEEDS, False),
    (["--bootstrap", "4097", "--bootstrap-quantiles", "0.5"], BQ_NEEDS, False),
    (["--isoforms"], ISO_NEEDS, False),
    (["--boundary-cut", "1e-6"], CUT_NEEDS, False),
    (["--asymptotic", "--boundary-cut", "-1"], CUT_RANGE, False),
    (["--asymptotic", "--boundary-cut", "nan"], CUT_RANGE, False),
    (["--presence-list", "none.list"], PRES_NEEDS, False),
    (["--profile-list", "none.list"], PROF_NEEDS, False),
    (["--profile-level", "0.9"], PROF_NEEDS, False),
    (["--profile-evals", "30"], PROF_NEEDS, False),
    (["--profile", "--profile-level", "0"], LEVEL_RANGE, False),
    (["--profile", "--profile-level", "1"], LEVEL_RANGE, False),
    (["--profile", "--profile-level", "nan"], LEVEL_RANGE, False),
    (["--compare-ratio", "2"], RATIO_NEEDS, False),
    (["--compare-list", "none.list"], LIST_NEEDS, False),
    (["-M", "--compare", "--compare-usage"], USAGE_G2T, True),
    (["--compare-usage"], USAGE_G2T, True),
    (["-M", "--compare", "--compare-ratio", "0"], RATIO_RANGE, False),
    (["-M", "--compare", "--compare-ratio", "-2"], RATIO_RANGE, False),
    (["-M", "--compare", "--compare-ratio", "inf"], RATIO_RANGE, False),
    (["-M", "--compare", "--compare-ratio", "nan"], RATIO_RANGE, False),
    (["--compare"], CMP_M, True),
    (["--compare-usage"] + G2T, UCMP_M, True),
    (["-s", "sideways"], "error: invalid strand type.", False),
]
# argument lists that trip two checks: the first of today's order is the one printed
FIRST = [
    (["-n", "0", "-e", "0"], "option -n must be a natural number.", False),                       # the switch reports in argument order
    (["-e", "0", "-n", "0"], "option -e must be positive.", False),
    (["--isoforms", "--bootstrap", "x"], BOOT, False),                                          # the switch before any cross-option check
    (["--subsample", "2", "--bootstrap-quantiles", "0.5"], SUB, False),
    (["--bootstrap-quantiles", "0.5", "--isoforms"], BQ_NEEDS, False),
    (["--isoforms", "--boundary-cut", "1"], ISO_NEEDS, False),
    (["--boundary-cut", "-1"], CUT_NEEDS, False),                                               # needs before range
    (["--boundary-cut", "1", "--presence-list", "l"], CUT_NEEDS, False),
    (["--presence-list", "l", "--profile-list", "l"], PRES_NEEDS, False),
    (["--profile-level", "2"], PROF_NEEDS, False),
    (["--profile", "--profile-level", "2", "--compare-ratio", "2"], LEVEL_RANGE, False),
    (["--compare-ratio", "-1"], RATIO_NEEDS, False),
    (["--compare-ratio", "2", "--compare-list", "l"], RATIO_NEEDS, False),
    (["--compare-list", "l", "--isoforms"], ISO_NEEDS, False),
    (["--compare-usage", "--compare", "--compare-ratio", "0"], USAGE_G2T, True),               # the gene map before the ratio's range
    (["--compare", "--compare-ratio", "0"], RATIO_RANGE, False),                                # ... and that before -M
    (["--compare", "--compare-usage"] + G2T, CMP_M, True),
    (["--compare", "-s", "sideways"], CMP_M, True),
    (["-s", "sideways", "--isoforms"], ISO_NEEDS, False),
]
ALL = SWITCH + COUNTS + SEEDS + LISTS + DEVICES + CROSS + FIRST


@pytest.fixture(scope="module", autouse=True)
def _built():
    _build.build_all()


def _cli(args, tmp_path, last="none.bowtie", positional=True):
    """as test_isoforms_cpu._cli: no device, an index that does not exist; the output directory is one that does not exist yet either"""
    tail = ["-I", str(tmp_path / "none.rsh"), str(tmp_path / "o"), "out", last] if positional else []
    return subprocess.run([_build.CLI] + args + ["-P"] + tail, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=60,
                          env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))


def _check(r, tmp_path, message, usage):
    assert r.returncode == 1
    head, sep, _ = r.stderr.partition("Usage : ")
    assert head == (message + "\n" if message else "") and bool(sep) == usage, r.stderr
    assert not (tmp_path / "o").exists() and r.stdout == ""                              # nothing made, nothing solved
    assert "none.rsh" not in r.stderr and (usage or "rsh" not in r.stderr)                # the check ran before any input was opened


@pytest.mark.parametrize("args,message,usage", ALL, ids=[" ".join(a)[:60] or "-" for a, _, _ in ALL])
def test_message(args, message, usage, tmp_path):
    _check(_cli(args, tmp_path), tmp_path, message, usage)


def test_a_repeated_list_option_starts_again(tmp_path):
    """--subsample and --bootstrap-quantiles replace an earlier list, so 64 + 1 entries over two options pass the parser; --devices
    appends, and stops reading without a word at 64 entries"""
    full = ",".join(["0.5"] * 64)
    for args in (["--subsample", full, "--subsample", "1"], ["--bootstrap", "8", "--bootstrap-quantiles", full, "--bootstrap-quantiles", "1"],
                 ["--devices", ",".join(["0"] * 65)], ["--devices", ",".join(["0"] * 64), "--devices", "x"], ["--devices", "0,"]):
        r = _cli(args, tmp_path)
        assert r.returncode == 1 and "wants a" not in r.stderr and "none.rsh" in r.stderr, args      # as far as the index


def test_in_range_values_reach_the_index(tmp_path):
    for args in (["--bootstrap", "0"], ["--bootstrap", "1000000"], ["--subsample-reps", "1"], ["--bootstrap-seed", "18446744073709551615"],
                 ["--subsample", "1"], ["--subsample", "1e-300,0.5"], ["--bootstrap", "4096", "--bootstrap-quantiles", "0,1"],
                 ["--devices", "0,1023"], ["--asymptotic", "--boundary-cut", "0"], ["--profile", "--profile-level", "0.5", "--profile-evals", "1"],
                 ["--count-floor", "0"]):
        r = _cli(args, tmp_path)
        assert r.returncode == 1 and "none.rsh" in r.stderr and "Usage" not in r.stderr, args


def test_usage_alone(tmp_path):
    """an unknown option, a missing index and too few arguments print the usage text and nothing of the driver's own before it"""
    r = _cli(["--no-such-option"], tmp_path)
    assert r.returncode == 1 and "Usage : " in r.stderr and "none.rsh" not in r.stderr and not (tmp_path / "o").exists()
    for args in ([], ["-I", str(tmp_path / "none.rsh"), str(tmp_path / "o"), "out"]):
        _check(_cli(args, tmp_path, positional=False), tmp_path, "", True)
    _check(_cli(["--isoforms"], tmp_path, positional=False), tmp_path, ISO_NEEDS, False)          # the cross-option checks come first


def test_sample_list_checks(tmp_path):
    """-M: a list that cannot be opened, an empty one, and --compare / --compare-usage with a one-line list"""
    _check(_cli(["-M"], tmp_path, last=str(tmp_path / "none.list")), tmp_path, "Can't open alignment list file.", False)
    empty, one = tmp_path / "empty.list", tmp_path / "one.list"
    empty.write_text("\n\r\n")
    one.write_text("\nnone.bowtie\n\n")
    _check(_cli(["-M"], tmp_path, last=str(empty)), tmp_path, "No alignment files in the alignment list", False)
    _check(_cli(["-M", "--compare"], tmp_path, last=str(empty)), tmp_path, "No alignment files in the alignment list", False)
    _check(_cli(["-M", "--compare"], tmp_path, last=str(one)), tmp_path, CMP_M, True)
    _check(_cli(["-M", "--compare-usage"] + G2T, tmp_path, last=str(one)), tmp_path, UCMP_M, True)
    _check(_cli(["-M", "--compare", "--compare-usage"] + G2T, tmp_path, last=str(one)), tmp_path, CMP_M, True)
    _check(_cli(["-M", "--compare", "-s", "sideways"], tmp_path, last=str(one)), tmp_path, "error: invalid strand type.", False)
    two = tmp_path / "two.list"
    two.write_text("none.bowtie\nnone.bowtie\n")
    r = _cli(["-M", "--compare", "--compare-usage"] + G2T, tmp_path, last=str(two))
    assert r.returncode == 1 and "none.rsh" in r.stderr and "needs" not in r.stderr
