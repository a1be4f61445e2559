"""The return codes of every batched call and plan helper on a fixed grid of arguments, without a GPU, against the codes recorded from
the commit before the calls' host side was moved onto batch_common.h's shared checks: sizes -1 ... 2^20, every row
stride around its width, every batch stride around its member, batch 0, 1 and 2, every pointer NULL and aliased onto every other
operand's first and last byte.  tools/record_batch_arg_codes.py holds the grid and is both the recorder and the comparer; it runs as a
process of its own because it hides the GPUs from the HIP runtime before the library loads (the grid's operands are addresses that
are never touched: a call that wrongly got past its checks must not be able to launch on them)."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORDER = os.path.join(ROOT, "tools", "record_batch_arg_codes.py")
FIXTURE = os.path.join(ROOT, "tests", "golden", "batch_arg_codes.json")


def test_every_batched_call_keeps_its_recorded_return_codes():
    r = subprocess.run([sys.executable, RECORDER, "--check", FIXTURE], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr


def test_the_fixture_covers_every_batched_entry_point_and_helper():
    """Every *_batch_dev entry point and every plan, units, slices and scratch helper of include/m4ri_amd.h's batched calls is in the
    fixture, with refusals, successes and both error codes among the recorded answers."""
    import m4ri_amd
    codes = json.load(open(FIXTURE))
    batched = [n for n in m4ri_amd.SYMBOLS if ("_batch" in n and n.endswith("_dev") or "_plan_" in n and "_batch" in n or n.endswith(("_units", "_slices", "_scratch_bytes")))
               and n not in ("m4ri_amd_m4rm_batch_dev", "m4ri_amd_mul_batch_dev")]  # the engine's batches: no *_batch.hip launcher
    assert sorted(batched) == sorted(codes)
    for name, c in codes.items():
        if name.endswith("_dev"):
            assert "1" in c and "0" in c and "?" not in c, name
    assert sum(len(c) for c in codes.values()) > 10000
