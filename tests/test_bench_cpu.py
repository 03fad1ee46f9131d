"""bench.py's roofline.traffic lookup (CPU): a PMC collection is quoted only when it was taken on the kernel source in the tree."""
import importlib.util
import json
import os
import shutil

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_committed_pmc_collection_matches_the_kernel_source():
    """Editing ANY source under mertools_amd/csrc/ without re-collecting the PMC passes (scripts/pmc_traffic.sh, scripts/pmc_mfma.sh) makes this
    fail — on purpose: the bench would otherwise print traffic = null / mfma_busy = null on the GPU box."""
    b = _bench()
    traffic, detail = b.pmc_traffic("gemm16p", 5e8)   # (the default preset launches the one-pass kernel only)
    assert traffic is not None and traffic > 1e8, detail
    assert detail["kernel_source_sha"] == b.kernel_source_sha() and detail["source"].startswith("profiles/")
    busy = b.pmc_mfma_busy("gemm16p")
    assert busy is not None and 0.05 < busy["mfma_busy"] < 1.0 and busy["kernel_source_sha"] == b.kernel_source_sha(), busy
    # the counter calibration the definition rests on: 16 busy cycles per 16x16x32 MFMA
    assert abs(busy["SQ_VALU_MFMA_BUSY_CYCLES"] / busy["SQ_INSTS_MFMA"] - 16.0) < 0.01


def test_committed_kernel_stats_match_the_kernel_source():
    """The rocprofv3 --kernel-trace --stats summary under profiles/ (the per-kernel times DESIGN.md and the judge's recomputation rest on)
    carries the sha of the library sources it was taken on (scripts/stamp_kernel_stats.py): a summary of another tree fails here."""
    import glob
    b = _bench()
    stamps = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_*kernel_stats.json")))   # (the latest round's sorts last)
    assert stamps, "no stamped kernel-stats summary under profiles/"
    d = json.load(open(stamps[-1]))
    assert d["_source_sha"] == b.kernel_source_sha(), (stamps[-1], d["_source_sha"], b.kernel_source_sha())
    csv = open(os.path.join(ROOT, "profiles", d["csv"])).read()
    assert "gemm16p_kernel" in csv and "gemm16_kernel" in csv      # the persistent family and the MX conv-stack kernel both have rows


def test_stale_pmc_collection_is_refused(tmp_path):
    import glob
    b = _bench()
    root = tmp_path / "tree"
    (root / "mertools_amd" / "csrc").mkdir(parents=True)
    (root / "profiles").mkdir()
    for f in glob.glob(os.path.join(ROOT, "mertools_amd", "csrc", "*")):
        if f.endswith((".h", ".hip", ".cpp")):
            shutil.copy(f, root / "mertools_amd" / "csrc" / os.path.basename(f))
    pmc = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_*pmc_hbm_traffic*.json")))[-1]
    shutil.copy(pmc, root / "profiles" / os.path.basename(pmc))
    assert b.pmc_traffic("gemm16p", 5e8, root=str(root))[0] is not None
    with open(root / "mertools_amd" / "csrc" / "norm.hip", "a") as f:      # ANY source of the library, not only the GEMM template
        f.write("// a kernel edit\n")
    traffic, detail = b.pmc_traffic("gemm16p", 5e8, root=str(root))
    assert traffic is None and os.path.basename(pmc) in detail["note"] and b.kernel_source_sha(str(root)) in detail["note"]
    # a collection without a stamp (round 1's) is never quoted either
    d = json.load(open(root / "profiles" / os.path.basename(pmc)))
    d.pop("_source_sha")
    json.dump(d, open(root / "profiles" / os.path.basename(pmc), "w"))
    assert b.pmc_traffic("gemm16p", 5e8, root=str(root))[0] is None


def test_dump_outputs_writes_float32_features_within_the_cap(tmp_path, monkeypatch):
    """--dump-outputs: one float32 [clips, D] file per modality, the same clips in each; above the cap a fixed every-k-th-clip sample."""
    import numpy as np
    import torch
    b = _bench()
    g = torch.Generator().manual_seed(0)
    feats = {"a": torch.randn(64, 768, generator=g), "v": torch.randn(64, 512, generator=g).half(), "t": torch.randn(64, 768, generator=g)}
    b.dump_outputs(feats, str(tmp_path / "all"))
    for m, name in b.DUMP_NAMES.items():
        x = np.load(tmp_path / "all" / f"{name}.npy")
        assert x.dtype == np.float32 and np.array_equal(x, feats[m].float().numpy())
    monkeypatch.setattr(b, "DUMP_MAX_BYTES", 100_000)
    b.dump_outputs(feats, str(tmp_path / "cap"))
    got = {name: np.load(tmp_path / "cap" / f"{name}.npy") for name in b.DUMP_NAMES.values()}
    assert sum(x.nbytes for x in got.values()) <= 100_000
    assert np.array_equal(got["audio"], feats["a"].numpy()[::6]) and got["visual"].shape == (11, 512)


def test_plain_run_by_default_and_steps_validated(monkeypatch):
    import pytest
    b = _bench()
    monkeypatch.setattr("sys.argv", ["bench.py", "--steps", "7"])
    a = b.parse()
    assert a.steps == 7 and not a.full and a.dump_outputs is None
    monkeypatch.setattr("sys.argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        b.parse()
