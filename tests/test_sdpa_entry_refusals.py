"""What the attention entries answer before any device work, call for call: tests/golden/sdpa_entry_refusals.json holds a corpus of calls to tf_sdpa_f16,
tf_sdpa_16, tf_sdpa_dual_16 and tf_sdpa_pag_16 that return before a launch (a null tensor, bad sizes, a bad head size, each misaligned stride in turn,
too many work items, a slice no kernel can address for each of k / v / k2 / v2, Tk2 > 64, a dual head size outside {40, 80, 160}, a perturbed batch
range outside [0, B], a null flag, B == 0 or Tq == 0, TF_SDPA_GENERIC refusing the dual and the perturbed form -- and pairs of these, which pin the order
of the checks) and to the host queries tf_sdpa_instance, tf_sdpa_dual_instance, tf_sdpa_pag_instance and tf_sdpa_split_ks over a grid of shapes that
names every TF_SDPA_INST_* value and both split forms.  Per call: the return value and, for a status, the whole tf_last_error() text.

Provenance: the answers are those of the library built at the commit BEFORE the attention units were taken apart into sdpa_common.h / sdpa_generic.h /
sdpa_dma.h (one translation unit per family), recorded there, where no GPU is visible, with `python tests/test_sdpa_entry_refusals.py` -- record mode
builds the corpus (corpus() below), answers every call with the library in the tree and writes the file.  The test replays it against the library in
the tree.  No call of the corpus may reach a launch (with placeholder pointers it would fault where a GPU is visible): the test checks that on the
recorded answers before it makes a single call, so it runs the same with and without a GPU."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sdpa_entry_refusals.json")
E_ARG, E_UNSUPPORTED = 10001, 10002

_T = ["q_sb", "q_sh", "q_st", "k_sb", "k_sh", "k_st", "v_sb", "v_sh", "v_st"]
_O = ["o_sb", "o_sh", "o_st"]
_T2 = ["k2_sb", "k2_sh", "k2_st", "v2_sb", "v2_sh", "v2_st"]
SIG = {     # the parameter lists of include/tinyfusers_hip.h
    "tf_sdpa_f16": ["o", "q", "k", "v", "B", "NH", "Tq", "Tk", "HS"] + _T + _O + ["causal", "s"],
    "tf_sdpa_16": ["dtype", "o", "q", "k", "v", "B", "NH", "Tq", "Tk", "HS"] + _T + _O + ["causal", "s"],
    "tf_sdpa_dual_16": ["dtype", "o", "q", "k", "v", "Tk", "k2", "v2", "Tk2", "scale2", "B", "NH", "Tq", "HS"] + _T + _T2 + _O + ["s"],
    "tf_sdpa_pag_16": ["dtype", "o", "q", "k", "v", "B", "NH", "Tq", "Tk", "HS"] + _T + _O + ["b0", "b1", "flag", "s"],
    "tf_sdpa_instance": ["dtype", "B", "NH", "Tq", "Tk", "HS", "k_st", "v_st", "causal"],
    "tf_sdpa_dual_instance": ["dtype", "B", "NH", "Tq", "Tk", "Tk2", "HS", "k_st", "v_st", "k2_st", "v2_st"],
    "tf_sdpa_pag_instance": ["dtype", "B", "NH", "Tq", "Tk", "HS", "k_st", "v_st", "b0", "b1"],
    "tf_sdpa_split_ks": ["B", "NH", "Tq", "Tk", "HS", "causal"],
}
FIELDS = ("fn", "kw", "ks", "env", "ret", "err")      # one call of the file, a list in this order
LAUNCHES = ("tf_sdpa_f16", "tf_sdpa_16", "tf_sdpa_dual_16", "tf_sdpa_pag_16")
POINTERS = ("o", "q", "k", "v", "k2", "v2", "scale2", "flag")


def _base(fn, **kw):
    """A well-formed call of `fn` as name -> value ("P": a placeholder pointer, None: NULL), contiguous (batch, head, token) strides, with kw on top."""
    a = dict(dtype=0, B=1, NH=2, Tq=200, Tk=77, Tk2=4, HS=40, causal=0, s=None, b0=0, b1=1)
    a.update({p: "P" for p in POINTERS})
    if fn == "tf_sdpa_pag_16" or fn == "tf_sdpa_pag_instance":
        a["Tk"] = 200                                       # self-attention
    a.update({k: v for k, v in kw.items() if k in ("B", "NH", "Tq", "Tk", "Tk2", "HS")})
    for t, n in (("q", a["Tq"]), ("k", a["Tk"]), ("v", a["Tk"]), ("k2", a["Tk2"]), ("v2", a["Tk2"]), ("o", a["Tq"])):
        a[t + "_sb"], a[t + "_sh"], a[t + "_st"] = a["NH"] * n * a["HS"], n * a["HS"], a["HS"]
    a.update(kw)
    return a


def corpus():
    """The calls, as {"fn", "kw" (what differs from _base(fn)), "ks" (tf_sdpa_force_split in front of the call), "env" (extra environment: the call runs in a child)}."""
    cases = []

    def add(fn, ks=0, env=None, **kw):
        cases.append({"fn": fn, "kw": {k: v for k, v in kw.items() if k in SIG[fn]}, "ks": ks, "env": env})
    big = dict(Tk=1 << 20)                                  # x a token stride of 1024 elements x 2 bytes = 2 GiB: beyond 32-bit byte offsets
    many = dict(B=1 << 20, NH=1 << 10, Tq=1 << 10)          # 2^34 (query block, head, batch) work items
    generic = {"TF_SDPA_GENERIC": "1"}
    # the launch entries.  tf_sdpa_16 in bfloat16 is tf_sdpa_f16's path compiled a second time: one call per check; the dual and the perturbed entry use
    # their dtype only behind the last refusal
    for fn, d in (("tf_sdpa_f16", {}), ("tf_sdpa_dual_16", dict(dtype=0)), ("tf_sdpa_pag_16", dict(dtype=0))):
        dual, pag = fn == "tf_sdpa_dual_16", fn == "tf_sdpa_pag_16"
        for p in [p for p in POINTERS if p in SIG[fn]]:
            add(fn, **{p: None}, **d)
        add(fn, o=None, HS=12, **d)                         # (pairs of faults pin the order of the checks)
        for kw in (dict(B=-1), dict(NH=0), dict(Tq=-1), dict(Tk=0), dict(Tk=-5, HS=12)):
            add(fn, **kw, **d)
        if dual:
            add(fn, Tk2=0, **d), add(fn, Tk2=65, **d), add(fn, Tk2=65, HS=64, **d), add(fn, Tk2=65, k2_st=44, **d), add(fn, Tk2=64, B=0, **d)
            for hs in (32, 64, 72, 128):
                add(fn, HS=hs, **d)
            add(fn, HS=64, q_sb=4, **d)
        if pag:
            for b0, b1 in ((-1, 1), (1, 0), (0, 2)):
                add(fn, b0=b0, b1=b1, **d)
            add(fn, b0=0, b1=2, q_sb=4, **d), add(fn, b0=0, b1=2, k_st=44, **d), add(fn, b0=0, b1=0, B=0, **d), add(fn, b0=0, b1=1, B=0, **d)
            add(fn, HS=72, **d), add(fn, HS=72, o_st=74, **d), add(fn, HS=72, Tq=0, **d)      # a head size of the generic kernel: no perturbed instance
        for hs in (0, 12, 168):
            add(fn, HS=hs, **d)
        add(fn, HS=12, k_st=44, **d), add(fn, **many, **d), add(fn, **many, q_sh=4, **d)
        for st in [n for n in SIG[fn] if n in _T + _T2]:
            add(fn, **{st: _base(fn)[st] + 4}, **d)
        add(fn, v_sb=4, o_sb=2, **d)
        for st in _O:
            add(fn, **{st: _base(fn)[st] + 2}, **d)
        add(fn, o_sh=2, B=0, **d)
        add(fn, B=0, **d), add(fn, Tq=0, **d), add(fn, B=0, **big, k_st=1024, **d)
        add(fn, **big, k_st=1024, **d), add(fn, **big, v_st=1024, **d), add(fn, **big, k_st=1024, HS=72, **d)
        if dual:
            add(fn, Tk2=64, k2_st=1 << 25, **d), add(fn, Tk2=64, v2_st=1 << 25, **d), add(fn, Tk2=64, k2_st=1 << 25, **big, v_st=1024, **d)
        if dual or pag:                                     # under TF_SDPA_GENERIC neither form has a kernel: refused, behind the other checks
            add(fn, env=generic, dtype=0), add(fn, env=generic, HS=80, B=2, NH=8, Tq=4096, dtype=1)
            add(fn, env=generic, q=None, **d), add(fn, env=generic, B=0, **d), add(fn, env=generic, **big, k_st=1024, **d)
            add(fn, dtype=2), add(fn, dtype=2, q=None), add(fn, dtype=1, **big, k_st=1024), add(fn, dtype=1, B=0)
    for kw in (dict(dtype=2), dict(dtype=-1), dict(dtype=2, q=None), dict(dtype=0, q=None), dict(dtype=0, HS=12), dict(dtype=0, B=0), dict(dtype=0, **big, k_st=1024)):
        add("tf_sdpa_16", **kw)
    for kw in (dict(v=None), dict(o=None, HS=12), dict(B=-1), dict(Tk=0), dict(HS=12), dict(HS=168), dict(HS=12, k_st=44), many, dict(q_sh=4, **many), dict(q_sb=4), dict(k_st=44),
               dict(v_sh=4), dict(v_sb=4, o_sb=2), dict(o_st=42), dict(o_sh=2, B=0), dict(B=0), dict(Tq=0), dict(B=0, k_st=1024, **big), dict(k_st=1024, **big), dict(v_st=1024, **big),
               dict(k_st=1024, HS=72, **big)):
        add("tf_sdpa_16", dtype=1, **kw)
    # the host queries: every shape at the per-shape rule, the shapes that split under every setting
    for b, nh, tq in [(1, 2, 200), (1, 128, 200), (1, 256, 256), (2, 8, 4096), (2, 8, 1024), (4, 8, 4096)]:
        for hs in (40, 72, 80, 160):
            for tk in (77, 4096) if hs in (40, 80) else (4096,):
                s = dict(B=b, NH=nh, Tq=tq, Tk=tk, HS=hs)
                variants = [(0, 0, 0)]
                if tk == 4096 and b == 2 and hs in (40, 80):
                    variants += [(1, 0, 0), (0, 1, 0), (0, 2, 0), (1, 2, 0), (0, 0, 1), (0, 2, 1)]
                for causal, ks, dtype in variants:
                    add("tf_sdpa_instance", ks=ks, causal=causal, dtype=dtype, **s)
                    if dtype == 0 and tk == 4096:
                        add("tf_sdpa_split_ks", ks=ks, causal=causal, **s)
            s = dict(B=b, NH=nh, Tq=tq, HS=hs)
            if hs != 72:
                add("tf_sdpa_pag_instance", Tk=tq, b1=b, **s), add("tf_sdpa_dual_instance", Tk=77, **s)
        add("tf_sdpa_pag_instance", ks=2, dtype=1, B=b, NH=nh, Tq=tq, Tk=tq, HS=80, b1=b), add("tf_sdpa_dual_instance", ks=2, dtype=1, B=b, NH=nh, Tq=tq, Tk=77, Tk2=64, HS=80)
    for fn in ("tf_sdpa_instance", "tf_sdpa_dual_instance", "tf_sdpa_pag_instance"):
        for kw in (dict(dtype=2), dict(dtype=-1, HS=12), dict(B=0), dict(Tq=0), dict(NH=0), dict(Tk=0), dict(HS=12), dict(HS=72), dict(HS=64),
                   dict(k_st=44), dict(v_st=44), dict(k_st=44, HS=12), dict(B=0, k_st=44), dict(Tk=1 << 20, k_st=1024), dict(Tk=1 << 20, v_st=1024), dict(Tk=1 << 20, k_st=1024, HS=72),
                   dict(Tk2=0), dict(Tk2=65), dict(Tk2=65, B=0), dict(Tk2=65, HS=64), dict(k2_st=44), dict(Tk2=64, k2_st=1 << 25), dict(Tk2=64, v2_st=1 << 25),
                   dict(Tk2=64, k2_st=1 << 25, Tk=1 << 20, k_st=1024), dict(b0=-1), dict(b0=1, b1=0), dict(b1=2), dict(b1=2, B=0)):
            if all(k in SIG[fn] for k in kw):               # (Tk2 / k2_st / v2_st: the dual query's, b0 / b1: the perturbed query's)
                add(fn, **kw)
        for kw in (dict(), dict(B=2, NH=8, Tq=4096, HS=80, b1=2), dict(B=0), dict(Tk=1 << 20, k_st=1024)):
            add(fn, env=generic, **kw)
    return cases


def _call(lib, case):
    a = _base(case["fn"], **case["kw"])
    args = [ctypes.c_void_p(4096) if a[n] == "P" else a[n] for n in SIG[case["fn"]]]
    assert lib.tf_sdpa_force_split(case["ks"]) == 0
    try:
        ret = getattr(lib, case["fn"])(*args)
    finally:
        lib.tf_sdpa_force_split(0)
    return {"ret": ret, "err": lib.tf_last_error().decode() if ret >= E_ARG else None}


def replay(lib, cases):
    """The answers of `lib` to `cases`, in their order; the cases with an environment of their own go to ONE child process per environment."""
    got = [None] * len(cases)
    envs = sorted({json.dumps(c["env"], sort_keys=True) for c in cases if c["env"]})
    for e in envs:
        idx = [i for i, c in enumerate(cases) if c["env"] and json.dumps(c["env"], sort_keys=True) == e]
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], input=json.dumps([cases[i] for i in idx]), capture_output=True, text=True,
                           env=dict(os.environ, **json.loads(e)), timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        for i, g in zip(idx, json.loads(r.stdout.strip().split("\n")[-1])):
            got[i] = g
    for i, c in enumerate(cases):
        if not c["env"]:
            got[i] = _call(lib, c)
    return got


def never_launches(case):
    """From the recorded answer alone: a launch entry answered with a refusal, or with TF_OK for a launch of no work (B == 0 or Tq == 0)."""
    if case["fn"] not in LAUNCHES:
        return True
    a = _base(case["fn"], **case["kw"])
    ret = case["expect"]["ret"]
    return ret in (E_ARG, E_UNSUPPORTED) or (ret == 0 and (a["B"] == 0 or a["Tq"] == 0))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    import tinyfusers_amd.native as n
    return n.lib


def test_the_entries_refuse_as_the_recorded_library_did(lib):
    cases = [dict(zip(FIELDS[:4], c[:4]), expect=dict(zip(FIELDS[4:], c[4:]))) for c in json.load(open(GOLDEN))["cases"]]
    assert [dict(c, expect=None) for c in cases] == [dict(c, expect=None) for c in corpus()]           # the file holds the corpus, whole and in order
    assert {c["fn"] for c in cases} == set(SIG)
    assert all(never_launches(c) for c in cases), [c for c in cases if not never_launches(c)][:3]         # checked BEFORE any call is made
    rets = {(c["fn"], c["expect"]["ret"]) for c in cases}
    assert {("tf_sdpa_instance", i) for i in (1, 2, 3, 4, 5)} <= rets and {("tf_sdpa_split_ks", 1), ("tf_sdpa_split_ks", 2)} <= rets
    assert {c["kw"]["HS"] for c in cases if c["fn"] == "tf_sdpa_instance" and c["expect"]["ret"] == 5} == {40, 80}                 # both split forms
    for fn in LAUNCHES:
        assert {(fn, E_ARG), (fn, E_UNSUPPORTED), (fn, 0)} <= rets, fn
    bad = [(i, c["fn"], c["kw"], c["ks"], c["env"], g, c["expect"]) for i, (c, g) in enumerate(zip(cases, replay(lib, cases))) if g != c["expect"]]
    assert not bad, (len(bad), bad[:5])


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    if "--child" in sys.argv:          # the calls that need an environment of their own: cases on stdin, answers on the last line of stdout
        import tinyfusers_amd.native as _native
        print(json.dumps([_call(_native.lib, c) for c in json.load(sys.stdin)]))
    else:                              # record mode
        import __graft_entry__
        __graft_entry__.build()
        import tinyfusers_amd.native as _native
        _n = ctypes.c_int(-1)
        assert not (_native.lib.tf_device_count(ctypes.byref(_n)) == 0 and _n.value > 0), "record where no GPU is visible"
        _cases = corpus()
        for _c, _g in zip(_cases, replay(_native.lib, _cases)):
            _c["expect"] = _g
        assert all(never_launches(_c) for _c in _cases), [_c for _c in _cases if not never_launches(_c)][:3]
        with open(GOLDEN, "w") as _f:
            _f.write('{"cases": [\n' + ",\n".join(json.dumps([_c[k] for k in FIELDS[:4]] + [_c["expect"][k] for k in FIELDS[4:]]) for _c in _cases) + "\n]}\n")
        print(len(_cases), "calls recorded")
