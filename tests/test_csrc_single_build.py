"""The native sources are compiled one way (no GPU, no build): no file under
cuda-surf_amd/csrc carries a preprocessor conditional, and neither those
files nor the Makefile nor tools/ name a SURF_DIAG_ diagnostic switch."""
from __future__ import annotations

import glob
import os
import re

from conftest import REPO

CSRC = sorted(p for p in glob.glob(os.path.join(REPO, "cuda-surf_amd", "csrc", "*")) if os.path.isfile(p))
BUILD = [os.path.join(REPO, "cuda-surf_amd", "Makefile")] + sorted(
    p for p in glob.glob(os.path.join(REPO, "tools", "*")) if os.path.isfile(p))
CONDITIONAL = re.compile(r"^\s*#\s*(if|ifdef|ifndef|elif|else|endif)\b")


def text(path: str) -> str:
    return open(path, errors="replace").read()


def test_csrc_has_no_preprocessor_conditionals():
    assert len(CSRC) >= 15
    hits = [f"{os.path.relpath(p, REPO)}:{n}: {line.strip()}" for p in CSRC
            for n, line in enumerate(text(p).splitlines(), 1) if CONDITIONAL.match(line)]
    assert not hits, hits


def test_no_diagnostic_switch_is_named():
    hits = [os.path.relpath(p, REPO) for p in CSRC + BUILD if "SURF_DIAG_" in text(p)]
    assert not hits, hits
