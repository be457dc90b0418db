"""CPU-side checks of the boundary: the C-ABI library builds/loads and exports exactly the symbols include/wtpse_hip.h
declares, and a definition that drifts from its declaration does not compile (no compute call is made without a GPU); the drop-in modules expose the reference's names, signatures and
state_dict keys; the product path fails loudly instead of falling back to the CPU."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import pytest
import torch

from test_oracle_golden import main_template, shape_template
from oracle.wtpse_cpu import DEFAULT_HPARAMS as HP

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"


def test_library_exports_every_declared_symbol():
    from wtpse_hip import build
    from wtpse_hip.lib import lib, parse_header, LIB_PATH
    build.build()                                   # no-op when up to date
    protos = parse_header()
    assert len(protos) >= 40
    dll = ctypes.CDLL(LIB_PATH)
    for name in protos:
        assert hasattr(dll, name), name
    assert set(lib().protos) == set(protos)
    # both directions: what the library exports under the ABI's prefix is what the header declares (any return type), nothing else
    text = re.sub(r"/\*.*?\*/", "", open(build.HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(wtpse_\w+)\s*\(", text))
    assert set(protos) <= declared and len(declared) >= len(protos)
    syms = subprocess.run([READELF, "--dyn-syms", "--wide", LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set()
    for line in syms.splitlines():
        f = line.split()
        if len(f) == 8 and f[6] != "UND" and f[4] in ("GLOBAL", "WEAK") and f[7].startswith("wtpse_"):
            exported.add(f[7].split("@")[0])
    assert exported == declared, (sorted(exported - declared), sorted(declared - exported))
    fn = dll.wtpse_source_hash
    fn.restype = ctypes.c_char_p
    assert fn().decode() == build.source_hash() == build.built_hash()
    # sizing helpers are host-only and may be called without a GPU
    L = lib()
    assert L.query("wtpse_conv_stats_blocks", 32, 256, 256) == 32 * 32 * 8
    assert L.query("wtpse_wgrad_ksplit", 32, 256, 256, 32, 32) == 512
    assert L.query("wtpse_wt_split", 32, 65536, 0) >= 1
    # launch geometry of the x3 convolutions at the benchmark's batch (rows of the statistics partials = tiles):
    # 256-pixel tiles where 64-channel blocks give two workgroups per CU ...
    assert L.query("wtpse_conv_x3_stats_blocks", 32, 128, 128, 64, 3) == 32 * 4 * 16       # up3.conv3: 8 x 32 tiles
    # ... 128-pixel tiles for the mid-sized launches (conv_x3r_k's 64-channel blocks on half tiles) and for the deepest level ...
    assert L.query("wtpse_conv_x3_stats_blocks", 32, 32, 32, 128, 3) == 32 * 1 * 8         # down3.conv2: 4 x 32 tiles
    assert L.query("wtpse_conv_x3_stats_blocks", 32, 16, 16, 256, 3) == 32 * 1 * 2         # down4.conv2: 8 x 16 tiles
    # ... but not for 1x1 convolutions (conv_x3_k only) nor for 32-channel layers with enough tiles
    assert L.query("wtpse_conv_x3_stats_blocks", 32, 32, 32, 128, 1) == 32 * 1 * 4
    assert L.query("wtpse_conv_x3_stats_blocks", 32, 256, 256, 32, 3) == 32 * 8 * 32
    # the register-resident weight gradient: maps a multiple of 32 wide, or 16 wide with 32-channel multiples (two images per step)
    assert L.query("wtpse_wgrad_r_supported", 64, 64, 3, 16, 64) == 1
    assert L.query("wtpse_wgrad_r_supported", 256, 256, 3, 16, 16) == 1
    assert L.query("wtpse_wgrad_r_supported", 16, 16, 3, 16, 16) == 0
    assert L.query("wtpse_wgrad_r_supported", 64, 64, 3, 16, 24) == 0
    assert L.query("wtpse_wgrad_r_slabs", 32, 16, 16, 256, 256) >= 1
    # argument validation happens before any launch
    assert L.raw("wtpse_conv_fwd")(0, 16, 0, 0, 0, 0, 0, 0, 0, 0, 0, 16, 0, 1, 8, 8, 16, 3, 0, 0, 0, 0) == -1


def test_drifted_declaration_does_not_compile(tmp_path):
    """Every translation unit is compiled against include/wtpse_hip.h, so a definition and a declaration that disagree are a
    compile error: here the header's copy declares wtpse_source_hash as returning int and abi.hip, which defines it, is checked
    against that copy (the unchanged header passes the same command)."""
    from wtpse_hip import build
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    cmd = [hipcc, "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", "-I", str(tmp_path), "-I", build.CSRC,
           "-I", os.path.dirname(build.HEADER), os.path.join(build.CSRC, "abi.hip")]
    text = open(build.HEADER).read()
    (tmp_path / "wtpse_hip.h").write_text(text)
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert text.count("const char* wtpse_source_hash(void);") == 1
    (tmp_path / "wtpse_hip.h").write_text(text.replace("const char* wtpse_source_hash(void);", "int wtpse_source_hash(void);"))
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode != 0
    assert "wtpse_source_hash" in res.stderr


def test_stale_library_is_refused(monkeypatch):
    """A library compiled from other sources than the tree's must not be bound (silent ABI mismatch otherwise)."""
    from wtpse_hip import build, lib as L
    build.build()
    monkeypatch.setattr(build, "source_hash", lambda: "0" * 32)
    with pytest.raises(L.WtpseError):
        L._Lib()


def test_dropin_surface_matches_reference():
    import algorithms
    import shape_networks
    assert algorithms.get_algorithm_class("WT_PSE") is algorithms.WT_PSE
    with pytest.raises(NotImplementedError):
        algorithms.get_algorithm_class("nope")
    sig = inspect.signature(algorithms.WT_PSE.__init__)
    assert list(sig.parameters)[1:] == ["n_channels", "n_classes", "hparams", "device", "two_step", "per_domain_batch",
                                        "source_domain_num", "feature_dim", "bilinear"]
    assert list(inspect.signature(algorithms.WT_PSE.update).parameters)[1:] == [
        "inputs", "mask", "step", "plot_show", "two_stage_inputs", "sp_mask", "two_step"]
    assert list(inspect.signature(algorithms.WT_PSE.predict).parameters)[1:] == ["learn_x_network", "inputs_all"]
    assert list(inspect.signature(shape_networks.ShapeVariationalDist_x.__init__).parameters)[1:] == [
        "hparams", "device", "n_classes", "number_source_domain", "batch_size"]
    assert list(inspect.signature(shape_networks.ShapeVariationalDist_x.update).parameters)[1:] == [
        "main_network", "inputs", "mask", "step", "plot_show", "two_stage_inputs", "two_step"]
    m = algorithms.WT_PSE(n_channels=3, n_classes=1, hparams=HP, device="cpu", two_step=False, per_domain_batch=2,
                          source_domain_num=3)
    s = shape_networks.ShapeVariationalDist_x(HP, "cpu", n_classes=1, number_source_domain=3, batch_size=2)
    for mod, tmpl in ((m, main_template()), (s, shape_template())):
        sd = mod.state_dict()
        assert list(sd.keys()) == list(tmpl.keys()) or set(sd.keys()) == set(tmpl.keys())
        for k, v in sd.items():
            assert tuple(v.shape) == tuple(tmpl[k].shape), k
    m0 = algorithms.WT_PSE(3, 1, dict(HP, whitening=False, shape_prior=False), "cpu", False)
    assert set(m0.state_dict().keys()) == set(main_template(False).keys())
    # attributes other objects reach into
    for attr in ("wt_model", "prior_dist", "attention_layer"):
        assert hasattr(m, attr)
    assert hasattr(m.prior_dist, "sample_forward") and hasattr(s, "sample_forward") and hasattr(s, "wt_model")


def test_no_cpu_fallback():
    import algorithms
    m = algorithms.WT_PSE(3, 1, HP, "cpu", False, per_domain_batch=1)
    x = torch.zeros(3, 3, 32, 32)
    with pytest.raises(RuntimeError):
        m.update(x, torch.zeros(3, 1, 32, 32), two_stage_inputs=x, two_step=True)
    with pytest.raises(NotImplementedError):
        algorithms.WT_PSE(3, 1, dict(HP, whitening=False), "cpu", False)      # mixed setting: broken in the reference too


def test_product_never_imports_oracle():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "wt-pse-code_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in src and "from oracle" not in src, os.path.join(dirpath, f)
