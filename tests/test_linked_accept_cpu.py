"""Host decisions of the linked bulk path (no GPU needed): the round state
(lz4ada_round_state.h) and laying a batch, accepting blocks and the plane modes
(lz4ada_linked_accept.h), through the stand-alone program that
checks them against a plain restatement of their rules."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OUTCOMES = ["all blocks accepted", "stop on a block code", "stop on a block checksum",
            "stop in a D1 round without a valid prediction", "stop outside a D1 round on an emulated block",
            "accepted because the prediction held", "stop at block 0"]


def test_linked_accept_against_its_restatement(tmp_path):
    """The stand-alone program, host code only, under the sanitizers, against the
    two headers alone: 400,000 random batches (fixed seed) over the round states,
    lengths, statuses and prediction flags its head lists.  Every one of the
    seven outcomes, counted by the restatement, is reached; the counts are the
    ones profiles/linked_accept_check.txt records."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "linked_accept_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-static-libasan", "-static-libubsan", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "bo-lz4-ada_amd", "csrc"),
                           os.path.join(ROOT, "tools", "linked_accept_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "400000 batches: no sanitizer report, every stage as restated" in r.stdout
    assert "FAIL" not in r.stdout
    for name in OUTCOMES:
        m = re.search("^" + re.escape(name) + r"\s+(\d+)$", r.stdout, re.M)
        assert m and int(m.group(1)) > 0, name
    with open(os.path.join(ROOT, "profiles", "linked_accept_check.txt")) as fh:
        assert fh.read() == r.stdout
