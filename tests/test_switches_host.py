"""CPU tests of the SURFHIP_* run-time switches: the one parser
(surfhip_switches_from_env, what a detector created now would read) with its
normalisations, and two guards against drift -- the library reads the
environment in one file only, and INTEGRATION.md's switch table names exactly
the variables the parser accepts."""
from __future__ import annotations

import glob
import os
import re

import pytest

# every switch with a valid value that is not its default, in the order the text lists them
CASES = [("SURFHIP_HESS_GATHER", "1"), ("SURFHIP_HESS_W", "0"), ("SURFHIP_Q01", "0"), ("SURFHIP_P0", "95"),
         ("SURFHIP_HESS_T0", "0"), ("SURFHIP_II_FUSE", "2"), ("SURFHIP_ROWSUM", "rowseg"), ("SURFHIP_DESC_UR", "1"),
         ("SURFHIP_TRACE_DESC", "0"), ("SURFHIP_ROT_ATOMIC", "1"), ("SURFHIP_SORT_BITONIC", "1"),
         ("SURFHIP_PREFETCH", "describe"), ("SURFHIP_DESC_BESIDE", "2"), ("SURFHIP_U2_LDSPAD", "4096"),
         ("SURFHIP_FIT_GRID", "640"), ("SURFHIP_FIT_CUBE", "0"), ("SURFHIP_II_BAND", "16"),
         ("SURFHIP_II_BAND_SMALL", "8")]
NAMES = [name for name, _ in CASES]


@pytest.fixture
def clean(monkeypatch):
    """No switch set (conftest sets two); SURFHIP_LIB_DIR is no switch and stays."""
    for name in os.environ:
        if name.startswith("SURFHIP_") and name != "SURFHIP_LIB_DIR":
            monkeypatch.delenv(name)
    return monkeypatch


def test_nothing_set_is_empty(surf, clean):
    clean.setenv("SURFHIP_LIB_DIR", os.path.dirname(surf.LIB_PATH))
    assert surf.switches_from_env() == ""


@pytest.mark.parametrize("name,value", CASES)
def test_each_switch_alone(surf, clean, name, value):
    clean.setenv(name, value)
    assert surf.switches_from_env() == f"{name}={value}"


def test_all_switches_in_table_order(surf, clean):
    for name, value in CASES:
        clean.setenv(name, value)
    assert surf.switches_from_env() == " ".join(f"{n}={v}" for n, v in CASES)


@pytest.mark.parametrize("name,value,text", [
    ("SURFHIP_II_BAND", "7", ""),                           # outside 8..64: dropped, the default holds
    ("SURFHIP_II_BAND", "64", "SURFHIP_II_BAND=64"),
    ("SURFHIP_II_BAND_SMALL", "33", ""),                    # outside 4..32
    ("SURFHIP_FIT_GRID", "10", "SURFHIP_FIT_GRID=64"),
    ("SURFHIP_P0", "77", "SURFHIP_P0=93"),
    ("SURFHIP_PREFETCH", "tail", "SURFHIP_PREFETCH=nms"),
    ("SURFHIP_ROT_ATOMIC", "0", "SURFHIP_ROT_ATOMIC=1"),    # on when set to anything
    ("SURFHIP_SORT_BITONIC", "", "SURFHIP_SORT_BITONIC=1"),
    ("SURFHIP_ROWSUM", "other", "SURFHIP_ROWSUM=p0"),
    ("SURFHIP_II_FUSE", "3", "SURFHIP_II_FUSE=1"),
])
def test_normalised(surf, clean, name, value, text):
    clean.setenv(name, value)
    assert surf.switches_from_env() == text


def test_text_is_cut_to_the_buffer(surf, clean):
    """The surfhip_hessian_plan convention: the full length comes back, buf holds what fits."""
    import ctypes as C
    clean.setenv("SURFHIP_P0", "95")
    buf = C.create_string_buffer(8)
    assert surf.lib.surfhip_switches_from_env(buf, len(buf)) == len("SURFHIP_P0=95")
    assert buf.value == b"SURFHIP"
    assert surf.lib.surfhip_switches_from_env(None, 0) == len("SURFHIP_P0=95")


def test_environment_is_read_in_one_file(surf):
    csrc = os.path.join(surf.REPO, "cuda-surf_amd", "csrc")
    files = sorted(glob.glob(os.path.join(csrc, "*")))
    assert len(files) >= 15
    readers = [os.path.basename(p) for p in files if any("getenv(" in line for line in open(p, errors="replace"))]
    assert readers == ["surfhip_api.hip"]


def test_integration_table_names_the_parsers_switches(surf):
    """The first column of INTEGRATION.md's switch table against the names the
    cases above exercise (each of which the parser gave back by name)."""
    rows = re.findall(r"^\| (`SURFHIP_[^|]*)\|", open(os.path.join(surf.REPO, "INTEGRATION.md")).read(), re.M)
    table = {name for row in rows for name in re.findall(r"SURFHIP_[A-Z0-9_]+", row)}
    assert table == set(NAMES) and len(NAMES) == 18
