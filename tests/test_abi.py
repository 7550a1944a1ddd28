"""The C ABI library: loads on a CPU-only host, exports every symbol include/*.h
declares, and its struct layouts agree with the ctypes mirror (and so with the Go
layout documented in INTEGRATION.md). No compute calls here (no GPU)."""
import re
import subprocess
from pathlib import Path

import pytest

from izpi_amd import _native as N

ROOT = Path(__file__).resolve().parents[1]


def declared_functions():
    names = set()
    for h in (ROOT / "include").glob("*.h"):
        txt = re.sub(r"/\*.*?\*/", "", h.read_text(), flags=re.S)
        names |= set(re.findall(r"^\s*(?:const\s+)?[a-z_0-9]+\s*\*?\s*(izpi_[a-z_0-9]+)\s*\(", txt, re.M))
    return names


def test_every_declared_symbol_is_exported():
    L = N.lib()
    decl = declared_functions()
    assert len(decl) >= 15
    missing = [n for n in sorted(decl) if not hasattr(L, n)]
    assert not missing, missing
    assert set(N.EXPORTS) == decl


def test_dynamic_symbol_table():
    out = subprocess.run(["nm", "-D", "--defined-only", str(N.LIB_PATH)], capture_output=True, text=True).stdout
    for name in declared_functions():
        assert re.search(r"\bT %s$" % name, out, re.M), name


def test_struct_layouts_match():
    import ctypes as C
    L = N.lib()
    for i, cls in enumerate(N.ABI_STRUCTS):
        assert L.izpi_abi_struct_size(i) == C.sizeof(cls), cls.__name__
    assert C.sizeof(N.BVH4Node) == 128  # == hitable.BVH4Node (bvh4.go:23-39)


def test_older_abi_requests_are_read_within_their_size(tmp_path):
    """request_copy and tuning_of (izpi_amd/csrc/izpi_req.h, the library's only readers of a
    caller's request as a whole) on heap blocks of exactly an older ABI's size, in a
    stand-alone program under AddressSanitizer and UBSan: no read past the caller's object,
    and a request below ABI 3 renders IZPI_ACC_RECURSIVE whatever lies behind it."""
    exe = tmp_path / "abi_prefix_check"
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(exe), str(ROOT / "tests" / "abi_prefix_check.cpp")], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stderr[-3000:]
    rows = {}
    for line in run.stdout.splitlines():
        name, *fields = line.split()
        rows[name] = dict(f.split("=") for f in fields)
    assert sorted(rows) == ["abi0", "abi0_no_tuning", "abi2", "abi3"]
    for name, r in rows.items():
        abi = 3 if name == "abi3" else 2 if name == "abi2" else 0
        assert r["abi"] == str(abi)
        # the caller's prefix, up to `tuning`
        assert (r["width"], r["height"], r["spp"], r["seed"], r["exposure"], r["tuning"]) == ("64", "48", "7", "12345", "1.5", "1")
        assert (int(r["sampler"]), int(r["post"])) == (N.SAMPLER_SPECTRAL, N.POST_SPECTRAL)
        assert int(r["accumulation"]) == (N.ACC_FORWARD if abi >= 3 else N.ACC_RECURSIVE) and r["pad_req"] == "0"
        # the tuning: ABI 1's ends at tail_paths, the later fields keep their defaults
        if name == "abi0_no_tuning":
            assert (r["slots"], r["flags"], r["tail_paths"], r["peer_timeout_ms"]) == ("0", "0", "0", "0")
        else:
            assert (r["slots"], int(r["flags"]), r["tail_paths"]) == ("300", N.TUNE_NO_TAIL, "99")
            assert r["peer_timeout_ms"] == ("4000" if abi >= 2 else "0")


def test_open_without_gpu_fails_cleanly():
    import ctypes as C
    try:
        import torch
        if torch.cuda.is_available():
            pytest.skip("a GPU is present")
    except Exception:
        pass
    ctx = C.c_void_p()
    assert N.lib().izpi_gpu_open(0, C.byref(ctx)) == N.IZPI_ERR_HIP
    assert not ctx.value


def test_product_does_not_import_oracle():
    for f in (ROOT / "izpi_amd").rglob("*.py"):
        assert not re.search(r"^\s*(from|import)\s+oracle\b", f.read_text(), re.M), f
    for f in (ROOT / "izpi_amd" / "csrc").glob("*"):
        assert "oracle/" not in f.read_text() and "liboracle" not in f.read_text(), f


def test_no_fma_contraction_in_device_code(tmp_path):
    """-ffp-contract=off must reach the device: a*b+c stays two roundings (A21)."""
    src = tmp_path / "probe.hip"
    src.write_text("#include <hip/hip_runtime.h>\n__global__ void k(const double* a, double* o)"
                   "{ int i = threadIdx.x; o[i] = a[i] * a[i+1] + a[i+2]; }\n")
    from izpi_amd import build
    asm = tmp_path / "probe.s"
    subprocess.run([build.HIPCC, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "--cuda-device-only", "-S",
                    "-o", str(asm), str(src)], check=True)
    text = asm.read_text()
    assert "v_mul_f64" in text and "v_add_f64" in text
    assert "v_fma_f64" not in text and "v_fmac_f64" not in text
