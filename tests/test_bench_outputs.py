"""bench.py --dump-outputs: the C of the last timed step as float .npy files (a fixed, seeded sample of the bits of C plus per-row figures
of every row), so that two builds can be compared output for output; and what a plain run (no --full) prints."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_outputs_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def words_to_bits(words, n):
    """[rows, ceil(n / 64)] uint64 words -> [rows, n] 0/1, column j = bit j % 64 of word j // 64."""
    return np.array([[(int(words[r, j // 64]) >> (j % 64)) & 1 for j in range(n)] for r in range(words.shape[0])], dtype=np.uint8)


def expected(words, n, group=1):
    bits = words_to_bits(words, n)
    m = bits.shape[0]
    pop = np.array([bits[g:g + group].sum() for g in range(0, m, group)], dtype=np.float64)
    fold = []
    for g in range(0, m, group):
        x = 0
        for r in range(g, min(m, g + group)):
            for j in range(words.shape[1]):
                x ^= int(words[r, j]) & (((1 << (n - 64 * j)) - 1) if n - 64 * j < 64 else (1 << 64) - 1)
        fold.append([x >> 32, x & 0xFFFFFFFF])
    return bits, pop, np.array(fold, dtype=np.float64)


def load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_is_the_valid_bits_of_every_row_and_a_seeded_row_sample(bench, tmp_path):
    m, n = 300, 1000                                             # 1000 = 15 words + 40 bits: the excess bits of the last word are not C
    words = np.random.default_rng(7).integers(0, 2 ** 64, size=(m, 16), dtype=np.uint64)
    calls = []

    def rows_of(r0, r1):
        calls.append((r0, r1))
        return words[r0:r1]
    bench.dump_outputs(str(tmp_path / "a"), rows_of, m, n)
    got = load(tmp_path / "a")
    bits, pop, fold = expected(words, n)
    assert set(got) == {"C_rows_sample", "C_rows_sample_index", "C_row_popcount", "C_row_xor_fold"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    idx = got["C_rows_sample_index"].astype(np.int64)
    assert len(idx) == min(m, bench.DUMP_ROWS) and np.all(np.diff(idx) > 0) and idx[-1] < m
    assert got["C_rows_sample"].dtype == np.float32 and np.array_equal(got["C_rows_sample"], bits[idx].astype(np.float32))
    assert np.array_equal(got["C_row_popcount"], pop) and np.array_equal(got["C_row_xor_fold"], fold)
    assert calls[0][0] == 0 and calls[-1][1] == m
    # the same C gives the same files; one flipped bit of C changes them; bits beyond column n change nothing
    bench.dump_outputs(str(tmp_path / "b"), lambda r0, r1: words[r0:r1], m, n)
    assert all(np.array_equal(v, load(tmp_path / "b")[k]) for k, v in got.items())
    other = words.copy()
    other[5, 15] ^= np.uint64(1 << 50)                           # beyond column 1000
    bench.dump_outputs(str(tmp_path / "c"), lambda r0, r1: other[r0:r1], m, n)
    assert all(np.array_equal(v, load(tmp_path / "c")[k]) for k, v in got.items())
    other[5, 3] ^= np.uint64(1 << 9)
    bench.dump_outputs(str(tmp_path / "d"), lambda r0, r1: other[r0:r1], m, n)
    assert load(tmp_path / "d")["C_row_popcount"][5] == pop[5] + (1 - 2 * bits[5, 3 * 64 + 9])


def test_dump_samples_columns_and_groups_rows_of_a_large_c(bench, tmp_path, monkeypatch):
    """Past the size limits the bit sample takes seeded columns too, and the per-row figures go to groups of consecutive rows."""
    monkeypatch.setattr(bench, "DUMP_ROWS", 8)
    monkeypatch.setattr(bench, "DUMP_SAMPLE_BITS", 8 * 100)
    monkeypatch.setattr(bench, "DUMP_MAX_GROUPS", 16)
    m, n = 70, 192
    words = np.random.default_rng(8).integers(0, 2 ** 64, size=(m, 3), dtype=np.uint64)
    bench.dump_outputs(str(tmp_path), lambda r0, r1: words[r0:r1], m, n)
    got = load(tmp_path)
    bits, pop, fold = expected(words, n, group=5)              # ceil(70 / 16) = 5 rows per group, 14 groups
    rows, cols = got["C_rows_sample_index"].astype(np.int64), got["C_cols_sample_index"].astype(np.int64)
    assert len(rows) == 8 and len(cols) == 100 and np.all(np.diff(cols) > 0)
    assert np.array_equal(got["C_rows_sample"], bits[rows][:, cols].astype(np.float32))
    assert got["C_row_popcount"].shape == (14,) and np.array_equal(got["C_row_popcount"], pop) and np.array_equal(got["C_row_xor_fold"], fold)


def test_dump_of_the_headline_product_stays_within_64_mb(bench):
    """65536^3 and the widest BASELINE product (n = 131072): the sample and the per-row figures, in bytes."""
    for m, n in ((65536, 65536), (131072, 131072), (1, 1 << 26), (1 << 26, 1)):
        r = min(m, bench.DUMP_ROWS)
        k = n if r * n <= bench.DUMP_SAMPLE_BITS else min(bench.DUMP_MAX_COLS, bench.DUMP_SAMPLE_BITS // r)
        g = -(-m // -(-m // bench.DUMP_MAX_GROUPS))
        total = 4 * r * k + 8 * r + (8 * k if k < n else 0) + 3 * 8 * g
        assert total <= 64 << 20, (m, n, total)


def _bench_line(args, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only_and_dumps_the_product(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR` without --full: the contract fields, none of the measurements beside the
    number, and the dumped C equal to the CPU oracle's product of the same seeded inputs (ragged: excess bits in the last word of a row)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cpu_libs
    from m4ri_amd.mzd import Mzd
    m, l, n, seeds = 1000, 777, 1500, (21, 22)
    out = _bench_line(["--gpus", "1", "--steps", "3", "--warmup", "1", "--dims", f"{m},{l},{n}", "--seeds", f"{seeds[0]},{seeds[1]}",
                       "--dump-outputs", str(tmp_path)])
    assert out["metric"] == "gf2_matmul_n3_equiv_bitops_per_sec" and out["unit"] == "bit-op/s" and out["higher_is_better"] is True
    assert out["dtype"] == "u64" and out["steps"] == 3 and out["warmup"] == 1 and out["n_gpus"] == 1
    assert out["ms_per_step"] > 0 and abs(out["value"] - float(m) * l * n / (out["ms_per_step"] * 1e-3)) <= 1e-6 * out["value"]
    assert not {"roofline", "roofline_schedule", "cpu_baseline", "api", "api_ms", "verified"} & set(out)
    C = cpu_libs.oracle().mul(None, Mzd.random(m, l, seeds[0]), Mzd.random(l, n, seeds[1]), 0)
    words = C.masked()
    got = load(tmp_path)
    rows = got["C_rows_sample_index"].astype(np.int64)
    bits = np.unpackbits(words[rows].view(np.uint8), axis=1, bitorder="little")[:, :n]
    assert np.array_equal(got["C_rows_sample"], bits.astype(np.float32))
    assert np.array_equal(got["C_row_popcount"], np.bitwise_count(words).sum(axis=1).astype(np.float64))
    x = np.bitwise_xor.reduce(words, axis=1)
    assert np.array_equal(got["C_row_xor_fold"][:, 0], (x >> np.uint64(32)).astype(np.float64))
    assert np.array_equal(got["C_row_xor_fold"][:, 1], (x & np.uint64(0xFFFFFFFF)).astype(np.float64))
