"""CPU: the status words of the seven output files that carry one (output.c keeps one table per family) are the names the Python side
gives the same numbers, and every number outside a family's range is written as "?"."""
import numpy as np
import pytest

from emsar_amd import _build, hip, hostlib


def _write(kind, path, status):
    """statuses through the writer of `kind`, one line each, every other column harmless -> the column that holds the word"""
    n = len(status)
    names = ["n%d" % k for k in range(n)]
    z, i = np.zeros(n), np.zeros(n, dtype=np.int32)
    if kind == "presence":
        hostlib.write_presence(path, names, z, z, z, status, i - 1, z)
        return 5
    if kind == "profile":
        hostlib.write_profile(path, names, z, z, z, z, status)
        return 6
    if kind == "gprofile":
        hostlib.write_gprofile(path, names, z, z, z, z, z, i, status)
        return 7
    if kind == "compare":
        hostlib.write_compare(path, names, z, z, z, z, z, status, i)
        return 7
    if kind == "gcompare":
        hostlib.write_gcompare(path, names, z, z, z, z, z, status, i, i)
        return 6
    if kind == "ucompare":
        hostlib.write_ucompare(path, names, ["g"], i, z, z, z, z, z, status, i, i)
        return 7
    if kind == "asym":
        hostlib.write_asym(path, names, z, z, z, z, z + 1.0, status, i - 1, z)
        return 6
    hostlib.write_gasym(path, names, z, z, status)
    return 3


@pytest.mark.parametrize("kind,words", [("presence", hip.PRESENCE_STATUS), ("profile", hip.PROFILE_STATUS), ("gprofile", hip.PROFILE_GENE_STATUS),
                                        ("compare", hip.COMPARE_STATUS), ("gcompare", hip.COMPARE_GENE_STATUS), ("ucompare", hip.USAGE_STATUS),
                                        ("asym", hip.ASYM_STATUS), ("gasym", hip.ASYM_STATUS)])
def test_status_words(kind, words, tmp_path):
    _build.build_all()
    n = len(words)
    path = str(tmp_path / ("a." + kind))
    column = _write(kind, path, list(range(n)) + [n, -1, 2 ** 31 - 1, -2 ** 31])
    got = [l.split("\t")[column] for l in open(path).read().splitlines()[1:]]
    assert got == list(words) + ["?"] * 4
