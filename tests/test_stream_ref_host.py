"""tests/gpu/spin.hip, the delay kernel of the caller-stream tests, builds for
gfx950 without a warning (-Wall -Werror) and exports its one entry point.  No
GPU is involved: nothing is launched."""
from __future__ import annotations

import os
import re

import stream_ref


def test_spin_builds_cleanly_and_exports_its_launcher():
    lib = stream_ref.spin_lib()
    assert os.path.basename(lib._name) == "libspin.so"
    assert lib.spin_launch.restype is not None


def test_spin_loop_is_bounded_by_a_constant():
    """The loop's counter is compared with a compile-time cap and written nowhere else, so the kernel
    ends even if the clock never advances (read from the source; never run that way)."""
    src = open(stream_ref.SPIN_SRC).read()
    cap = re.search(r"static constexpr int kSpinCap = 1 << (\d+);", src)
    assert cap and 10 <= int(cap.group(1)) <= 22
    assert "for (int turn = 0; turn < kSpinCap; ++turn)" in src
    body = src.split("for (int turn = 0; turn < kSpinCap; ++turn)")[1].split("}")[0]
    assert "turn" not in body and not re.search(r"\b(while|goto|do)\b", src)
    assert "<<<1, 64, 0, (hipStream_t)stream>>>" in src
