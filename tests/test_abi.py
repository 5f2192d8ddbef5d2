"""CPU checks of the drop-in boundary: the C-ABI library loads without a GPU and exports every symbol that
include/tinyfusers_hip.h declares; argument validation and the status -> RuntimeError convention work."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def native():
    import __graft_entry__
    __graft_entry__.build()          # hipcc cross-compiles gfx950 without a GPU
    import tinyfusers_amd.native as n
    return n


def test_header_symbols_exported(native):
    hdr = open(os.path.join(ROOT, "include", "tinyfusers_hip.h")).read()
    names = sorted(set(re.findall(r"\b(tf_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))))
    assert len(names) >= 55
    assert sorted(native.declared_symbols()) == names
    dll = ctypes.CDLL(native.LIB_PATH)
    for n in names:
        assert hasattr(dll, n), f"{n} declared in the header but not exported by the library"


def test_patch_query_answers_with_the_launchers_rule(native):
    """tf_conv2d_patch_admits (host code): what lets a test tell k_igemm_patch from the deep ring it silently gives way to -- 3 x 3 / stride 1 /
    pad 1 on the 64-channel grid, W a power of two inside the tile, tiles {64, 128} x {128, 160}."""
    q = native.lib.tf_conv2d_patch_admits
    assert q(2, 16, 16, 64, 0, 320, 3, 3, 1, 1, 0, 0, 0, 64, 128) == 1 and q(2, 16, 16, 64, 64, 320, 3, 3, 1, 1, 0, 64, 0, 128, 160) == 1
    for bad in [(2, 16, 16, 64, 0, 320, 1, 1, 1, 0, 0, 0, 0, 64, 128), (2, 16, 16, 64, 0, 320, 3, 3, 1, 1, 0, 0, 0, 64, 64), (2, 10, 10, 64, 0, 320, 3, 3, 1, 1, 0, 0, 0, 64, 128),
                (2, 16, 16, 72, 0, 320, 3, 3, 1, 1, 0, 0, 0, 64, 128), (2, 16, 16, 64, 0, 320, 3, 3, 2, 1, 0, 0, 0, 64, 128), (2, 16, 16, 64, 0, 320, 3, 3, 1, 1, 1, 0, 0, 64, 128),
                (0, 16, 16, 64, 0, 320, 3, 3, 1, 1, 0, 0, 0, 64, 128), (2, 256, 256, 64, 0, 320, 3, 3, 1, 1, 0, 0, 0, 64, 128)]:
        assert q(*bad) == 0, bad


def test_ring_form_query_answers_with_the_launchers_rule(native):
    """tf_gemm_ring_form (host code): the k_igemm form a tile runs for an asked variant -- no wide ring on 128 x 160 and 256 x 128, no all-8 ring
    on 256 x 128 or off the 64-channel grid; what a tile has not runs the deep ring."""
    q = native.lib.tf_gemm_ring_form
    for bm in (64, 128):
        for bn in (64, 128, 160):
            assert q(bm, bn, 0, 1) == 0 and q(bm, bn, 3, 1) == 3 and q(bm, bn, 3, 0) == 0
            assert q(bm, bn, 1, 1) == q(bm, bn, 1, 0) == (0 if (bm, bn) == (128, 160) else 1)
    assert [q(256, 128, v, 1) for v in (0, 1, 3)] == [0, 0, 0]
    assert q(256, 160, 0, 1) == 10001 and q(64, 64, 2, 1) == 10001 and b"tf_gemm_ring_form" in native.lib.tf_last_error()


def test_every_entry_cites_the_reference():
    hdr = open(os.path.join(ROOT, "include", "tinyfusers_hip.h")).read()
    # each block of prototypes is preceded by a comment naming the reference file:line it replaces
    assert len(re.findall(r"[a-z_/]+\.(?:py|cu):\d+", hdr)) >= 30


def test_status_convention_without_gpu(native):
    n = ctypes.c_int(-1)
    rc = native.lib.tf_device_count(ctypes.byref(n))
    if rc == 0 and n.value > 0:
        pytest.skip("a GPU is visible: error-path check not applicable")
    assert n.value == 0
    with pytest.raises(RuntimeError, match=r"tf_init failed with status \d+"):
        native.hip.tf_init(0)
    assert native.lib.tf_last_error()          # human-readable reason travels with the status
    # argument validation happens before any device work
    assert native.lib.tf_linear_f16(None, None, None, None, None, 4, 4, 8, 0, None, 0, None) == 10001
    assert b"null tensor" in native.lib.tf_last_error()
    assert native.lib.tf_sdpa_f16(*([ctypes.c_void_p(8)] * 4), 1, 1, 4, 4, 12, *([8] * 12), 0, None) == 10001   # HS % 8
    assert native.lib.tf_version() >= 100


GEMM_ENTRY_TRACE = os.path.join(ROOT, "tests", "golden", "gemm_entry_trace.json")


def _replay_gemm_entry(lib, case, trace_path):
    """One call of the corpus: "P" is a non-null placeholder pointer (nothing dereferences it on the host), None is NULL, "I" an int the entry may
    write.  What the call shows without a device: its return value, the shape key it looked up (none when it returned first), the values left in
    its int out-arguments and, for TF_E_INVALID_VALUE, the entry name its message begins with."""
    outs = []

    def arg(a):
        if a == "P":
            return ctypes.c_void_p(4096)
        if a == "I":
            outs.append(ctypes.c_int(-7))
            return ctypes.byref(outs[-1])
        return a
    args = [arg(a) for a in case["args"]]
    assert lib.tf_gemm_tune_trace(1) == 0                  # (switching the trace on forgets the keys of the call before)
    ret = getattr(lib, case["fn"])(*args)
    assert lib.tf_gemm_tune_trace_dump(trace_path.encode()) == 0
    keys = [[int(v) for v in line.split()[:10]] for line in open(trace_path)]
    assert len(keys) <= 1, keys
    return {"ret": ret, "key": keys[0] if keys else None, "who": lib.tf_last_error().decode().split(":")[0] if ret == 10001 else None,
            "outs": [o.value for o in outs]}


def _replay_gemm_entries(native, cases, trace_path, with_placeholders):
    import sys
    mode = sys.modules["tinyfusers_amd.native.hip"]._mode
    try:
        assert native.lib.tf_gemm_autotune(2) == 0         # table only: a launch looks its key up and never tunes
        return [_replay_gemm_entry(native.lib, c, trace_path) if with_placeholders or not c["device"] else None for c in cases]
    finally:
        native.lib.tf_gemm_tune_trace(0)
        native.lib.tf_gemm_autotune(int(mode) if mode else 1)


def test_entries_describe_the_same_gemm_problems(native, tmp_path):
    """Which problem each conv / linear entry describes to the dispatcher: tests/golden/gemm_entry_trace.json holds a corpus of entry calls and,
    per call, what the library of the commit before the launch descriptors got their builders answered (python tests/test_abi.py records it).
    resolve() looks the shape key up before anything touches a device, so a well-formed call with placeholder pointers leaves its key in the
    trace and returns a status (not in the table, or no device); those calls ("device": true) run only where no GPU is visible.  The rejected
    calls and the host-only predicates return before any device work and run everywhere."""
    n = ctypes.c_int(-1)
    have_gpu = native.lib.tf_device_count(ctypes.byref(n)) == 0 and n.value > 0
    cases = json.load(open(GEMM_ENTRY_TRACE))["cases"]
    assert all(c["device"] or c["expect"]["key"] is None for c in cases)      # what runs next to a GPU never got as far as a launch
    got = _replay_gemm_entries(native, cases, str(tmp_path / "trace.txt"), not have_gpu)
    for i, (c, g) in enumerate(zip(cases, got)):
        assert g is None or g == c["expect"], (i, c["fn"], c["args"], g, c["expect"])
    if have_gpu:
        pytest.skip("a GPU is visible: the placeholder-pointer calls were not replayed (the rejected calls and predicates passed)")


def test_no_cpu_fallback(native, monkeypatch):
    """The product path must fail loudly when the HIP extension is missing."""
    import sys
    h = sys.modules["tinyfusers_amd.native.hip"]     # the module (the package attribute `hip` is the shim instance)
    monkeypatch.setattr(h, "LIB_PATH", "/nonexistent/libtinyfusers_hip.so")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        h._load()


def test_product_never_imports_the_oracle():
    import subprocess, sys
    out = subprocess.run(["grep", "-rlE", r"^\s*(from|import)\s+oracle", os.path.join(ROOT, "tinyfusers_amd")], capture_output=True, text=True)
    assert out.stdout.strip() == "", out.stdout


def test_shipped_library_holds_no_ablation_kernel(native):
    """Kernels that skip work and return wrong results by design (the DBG template instances tools/*_dbg.py time) are compiled only under
    -DTF_ABLATION into a second library; the shipped code objects hold none, no environment variable can select one, and the ablation
    bits of tf_gemm_debug are refused (one code path per op, as attention/sdpa.py:53-77 of the reference has)."""
    import sys
    sys.path.insert(0, ROOT)
    from tools.kernel_regs import LLVM, census
    if not os.path.exists(os.path.join(LLVM, "clang-offload-bundler")):
        pytest.skip("llvm tools not found")
    ks = census(os.path.dirname(native.LIB_PATH))
    assert 200 <= len(ks) <= 400, len(ks)                       # (round 5: every MFMA kernel in float16 and in bfloat16)
    for k in ks:
        m = re.match(r"void k_igemm_pp<(\d+), (\d+), (true|false), (true|false),", k["name"])
        assert not (m and m.group(4) == "true"), k["name"]                    # k_igemm_pp<BN, NP, FASTA, DBG, ...>
        m = re.match(r"void k_sdpa_dma<(\d+), (\d+), (\d+), (\d+), (true|false)>", k["name"])
        assert not k["name"].startswith("void k_sdpa_dma<") or (m and m.group(3) == "0"), k["name"]   # k_sdpa_dma<HS, QT, DBG, NW, BF>
        assert k["vspill"] == 0 and k["scratch"] == 0, k                      # no kernel spills vector registers
    assert native.lib.tf_gemm_debug(1) == 10001 and b"TF_ABLATION" in native.lib.tf_last_error()
    assert native.lib.tf_gemm_debug(512) == 0 and native.lib.tf_gemm_debug(0) == 0   # (variant selection is a test hook, not an ablation)
    src = open(os.path.join(ROOT, "tinyfusers_amd", "csrc", "sdpa.hip")).read()
    assert re.search(r"#ifdef TF_ABLATION\s*\nstatic int g_sdpa_dbg = getenv", src)   # TF_SDPA_DBG is read by the ablation build only


def test_host_code_is_clean_under_asan_ubsan():
    """SURVEY 5 "race detection / sanitizers": the host side of the library (table loader, run_gemm's tile logic, shape predicates, status
    paths, tf_rtc_* / tf_comm_* argument handling) under AddressSanitizer + UndefinedBehaviorSanitizer -- `python -m tinyfusers_amd.build
    --asan-host` builds lib/libtinyfusers_hip_asan.so (device code unsanitised; CPU container only), tests/aux/host_sanitizer_drive.py drives
    it in a child process with the ASan runtime preloaded; any finding aborts the child.  Skips where that library has not been built."""
    import subprocess
    import sys
    from tinyfusers_amd import build as b
    if not os.path.exists(b.LIB_ASAN):
        pytest.skip("lib/libtinyfusers_hip_asan.so not built (python -m tinyfusers_amd.build --asan-host)")
    srcs = [os.path.join(b.CSRC, f) for f in os.listdir(b.CSRC)]
    if any(os.path.getmtime(f) > os.path.getmtime(b.LIB_ASAN) for f in srcs):
        pytest.skip("lib/libtinyfusers_hip_asan.so is older than the sources: rebuild it with --asan-host")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "aux", "host_sanitizer_drive.py")], env=b.sanitizer_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "HOST_SANITIZER_OK" in r.stdout, (r.stdout[-1500:], r.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-4000:]


if __name__ == "__main__":       # record mode: answer every call of the corpus with the library in the tree and write the answers back
    import sys
    import tempfile
    sys.path.insert(0, ROOT)
    import __graft_entry__
    __graft_entry__.build()
    import tinyfusers_amd.native as _native
    _n = ctypes.c_int(-1)
    assert not (_native.lib.tf_device_count(ctypes.byref(_n)) == 0 and _n.value > 0), "record where no GPU is visible"
    _fx = json.load(open(GEMM_ENTRY_TRACE))
    with tempfile.TemporaryDirectory() as _d:
        for _c, _g in zip(_fx["cases"], _replay_gemm_entries(_native, _fx["cases"], os.path.join(_d, "trace.txt"), True)):
            _c["expect"] = _g
    with open(GEMM_ENTRY_TRACE, "w") as _f:
        _f.write('{"cases": [\n' + ",\n".join(json.dumps(_c) for _c in _fx["cases"]) + "\n]}\n")
