"""The library's BOFI_* knobs: one table (csrc/bofi_knobs.h), one reader (csrc/knobs.hip).

(a) the table and its reader as a stand-alone host program (tests/knobs_check.cpp: the header and its storage file, compiled with the system C++
    compiler, once more under AddressSanitizer / UBSan), run as a child process under a set environment;
(b) the sources as text: getenv in the reader only, the reload generation declared once, every BOFI_* name a row of the table, every row read."""
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "boficap_amd", "csrc")

# name: (kind, default, when) -- what each use site of the library read before there was a table (the defaults a launch has always seen)
EXPECTED = {
    "BOFI_RB_MIN_ROWS": ("INT", 4096, "RELOAD"), "BOFI_RB_ATTN": ("INT", 1, "RELOAD"), "BOFI_RB_ATTN_W": ("INT", 0, "RELOAD"),
    "BOFI_RB_ATTN_PROJ": ("INT", 1, "RELOAD"), "BOFI_RB_ATTN_SPLIT": ("INT", 1, "RELOAD"), "BOFI_RB_ATTN_SPLIT_MIN_B": ("INT", 512, "RELOAD"),
    "BOFI_RB_ATTN_SPLIT_WHICH": ("INT", 3, "RELOAD"), "BOFI_RB_GEMM": ("INT", 1, "RELOAD"), "BOFI_RB_FFN": ("INT", 1, "RELOAD"),
    "BOFI_RB_FFN_PROJ": ("INT", 1, "RELOAD"), "BOFI_RB_FFN_PROJ_MAXN": ("INT", 0, "RELOAD"), "BOFI_GEN_PAD": ("INT", 1, "RELOAD"),
    "BOFI_FILL_QKV_TAB": ("INT", 1, "RELOAD"), "BOFI_REFINE_IDS_ONLY": ("INT", 1, "RELOAD"), "BOFI_BOUND_LOOP": ("INT", 1, "RELOAD"),
    "BOFI_BOUND_LEAN": ("INT", 1, "RELOAD"), "BOFI_TAIL_DBG": ("INT", 0, "RELOAD"), "BOFI_DBG_PART": ("INT", 0, "RELOAD"),
    "BOFI_BOUND_DENSE": ("INT", 0, "CREATE"), "BOFI_SAIC_CACHE": ("INTP", 1, "CREATE"), "BOFI_SAIC_LEAN": ("INTP", 1, "CREATE"),
    "BOFI_EXP_SKIP": ("STR", 0, "RELOAD"), "BOFI_EXP_ITERS": ("INTP", 0, "RELOAD"),
    "BOFI_RB_FFN_V": ("INTP", 5, "RELOAD"), "BOFI_RB_FFN_BPW": ("INT", 1, "RELOAD"), "BOFI_RB_FFN_ONE": ("INT", 1, "RELOAD"),
    "BOFI_RB_FFN_V5_ROWS": ("INT", 0, "RELOAD"), "BOFI_RB_GEMM_MT": ("INT", 6, "RELOAD"), "BOFI_RB_GEMM_MT8_ROWS": ("INT", 4096, "RELOAD"),
    "BOFI_RB_GEMM_MT_MIN_N": ("INT", 0, "RELOAD"), "BOFI_RB_GEN_MT6": ("INTP", -1, "RELOAD"), "BOFI_VOCAB_MT": ("INT", 4, "RELOAD"),
    "BOFI_VOCAB_SPLIT": ("INT", 0, "RELOAD"), "BOFI_RB_DBG": ("INT", 0, "RELOAD"),
    "BOFI_GEMM_TILE": ("STR", 0, "RELOAD"), "BOFI_GEMM_HEUR2": ("INT", 1, "RELOAD"), "BOFI_GEMM_DEEP": ("INT", 1, "RELOAD"),
    "BOFI_GEMM_BANDS": ("INT", 0, "RELOAD"), "BOFI_GEMM_DBG": ("INT", 0, "RELOAD"), "BOFI_GEMM_DBG_BUF": ("STR", 0, "RELOAD"),
    "BOFI_GEMM_PERS": ("INT", 1, "RELOAD"), "BOFI_GEMM_PERS_MIN": ("INT", 90, "RELOAD"), "BOFI_GEMM_PERS_BM128": ("INT", 128, "RELOAD"),
    "BOFI_GEMM_PERS_GRID": ("INT", 256, "RELOAD"), "BOFI_GEMM_PERS_ROUNDS": ("INT", 1, "RELOAD"), "BOFI_GEMM_PERS_FAST": ("INT", 1, "RELOAD"),
    "BOFI_TN_WT": ("INT", 0, "RELOAD"), "BOFI_TN_WGS": ("INT", 0, "RELOAD"), "BOFI_ROWGEMM_NT": ("INT", 0, "RELOAD"),
    "BOFI_ATTN_GENERIC": ("INTP", 0, "RELOAD"), "BOFI_TAIL_SMALL_AT": ("INT", 65, "RELOAD"), "BOFI_BL_DBG": ("INT", 0, "RELOAD"),
    "BOFI_BL_PAIR": ("INT", 1, "RELOAD"), "BOFI_BL_PAIR_MAX_B": ("INT", 384, "RELOAD"),
}
ROW = re.compile(r'^\s*X\((BOFI_[A-Z0-9_]+), (INT|INTP|STR), (-?\d+), (RELOAD|CREATE), "(.+)"\)', re.M)


def _table_rows():
    return {m.group(1): (m.group(2), int(m.group(3)), m.group(4)) for m in ROW.finditer(open(os.path.join(CSRC, "bofi_knobs.h")).read())}


def _compile(out, *flags):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no system C++ compiler"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, f"-I{CSRC}", os.path.join(ROOT, "tests", "knobs_check.cpp"), "-o", out]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    return out


@pytest.fixture(scope="module", params=["plain", "asan-ubsan"])
def prog(request, tmp_path_factory):
    d = tmp_path_factory.mktemp("knobs_" + request.param.replace("-", "_"))
    # (the sanitizer runtimes linked INTO the program: it is a stand-alone host program and needs nothing from its environment)
    flags = () if request.param == "plain" else ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan")
    return _compile(str(d / "knobs_check"), *flags)


def _run(prog, *args, **env):
    clean = {k: v for k, v in os.environ.items() if not k.startswith("BOFI_")}
    p = subprocess.run([prog, *args], capture_output=True, text=True, env=dict(clean, **env), timeout=60)
    assert p.returncode == 0, (p.returncode, p.stdout[-1000:], p.stderr[-3000:])
    return p.stdout.splitlines()


def _dump(prog, **env):
    out = {}
    for line in _run(prog, "dump", **env):
        name, kind, when, dflt, value, is_set, text = line.split("|")
        out[name] = dict(kind=kind, when=when, dflt=int(dflt), value=int(value), set=int(is_set), text=None if text == "-" else text)
    return out


def test_the_table_in_the_header_is_the_expected_one():
    assert _table_rows() == EXPECTED


def test_every_row_has_its_default_when_nothing_is_set(prog):
    rows = _dump(prog)
    assert list(rows) == list(_table_rows())                     # the compiled table is the header's, in its order
    for name, (kind, dflt, when) in EXPECTED.items():
        r = rows[name]
        assert (r["kind"], r["when"], r["dflt"]) == (kind, when, dflt), name
        assert r["value"] == dflt and r["set"] == 0 and r["text"] is None, name


def test_set_values_presence_and_strings(prog):
    rows = _dump(prog, BOFI_RB_MIN_ROWS="0", BOFI_GEMM_PERS_MIN="1", BOFI_BL_PAIR_MAX_B="-7", BOFI_RB_FFN_V="0", BOFI_RB_GEN_MT6="0", BOFI_SAIC_CACHE="0",
                 BOFI_ATTN_GENERIC="0", BOFI_SAIC_LEAN="1", BOFI_GEMM_TILE="128x64x2x8", BOFI_GEMM_DBG_BUF="0x7f0012345000", BOFI_EXP_SKIP="attn,ffn")
    assert rows["BOFI_RB_MIN_ROWS"]["value"] == 0 and rows["BOFI_GEMM_PERS_MIN"]["value"] == 1 and rows["BOFI_BL_PAIR_MAX_B"]["value"] == -7
    # presence kinds: "0" is a value and SET; unset is the default and NOT set
    for name, value in (("BOFI_RB_FFN_V", 0), ("BOFI_RB_GEN_MT6", 0), ("BOFI_SAIC_CACHE", 0), ("BOFI_ATTN_GENERIC", 0), ("BOFI_SAIC_LEAN", 1)):
        assert rows[name]["value"] == value and rows[name]["set"] == 1, name
    assert rows["BOFI_EXP_ITERS"]["set"] == 0 and rows["BOFI_EXP_ITERS"]["value"] == 0
    assert rows["BOFI_GEMM_TILE"]["text"] == "128x64x2x8" and rows["BOFI_GEMM_DBG_BUF"]["text"] == "0x7f0012345000" and rows["BOFI_EXP_SKIP"]["text"] == "attn,ffn"
    # every row that was not set keeps its default
    touched = {"BOFI_RB_MIN_ROWS", "BOFI_GEMM_PERS_MIN", "BOFI_BL_PAIR_MAX_B", "BOFI_RB_FFN_V", "BOFI_RB_GEN_MT6", "BOFI_SAIC_CACHE", "BOFI_ATTN_GENERIC",
               "BOFI_SAIC_LEAN", "BOFI_GEMM_TILE", "BOFI_GEMM_DBG_BUF", "BOFI_EXP_SKIP"}
    for name, (_, dflt, _) in EXPECTED.items():
        if name not in touched:
            assert rows[name]["value"] == dflt and rows[name]["set"] == 0, name


@pytest.mark.parametrize("name,start,new", [("BOFI_RB_FFN_V", None, "2"), ("BOFI_RB_MIN_ROWS", "17", "0"), ("BOFI_GEMM_TILE", None, "64x64x4x8"),
                                            ("BOFI_GEMM_TILE", "64x64x2x8", "128x128x3x8"), ("BOFI_SAIC_CACHE", None, "0")])
def test_a_change_is_seen_by_the_reload_and_not_before(prog, name, start, new):
    kind, dflt, _ = EXPECTED[name]

    def want(text):                # value, set, text of the row with the variable at `text`
        if text is None:
            return [str(dflt), "0", "-"]
        return [str(dflt if kind == "STR" else int(text)), "1", text]

    lines = dict(l.split(" ", 1) for l in _run(prog, "reload", name, new, **({name: start} if start is not None else {})))
    assert lines["first"].split() == want(start)
    assert lines["stale"].split() == want(start)                 # setenv after the first use: the table keeps the value of the last load ...
    assert lines["live"].split() == want(new)                    # ... the live read (rows read at engine creation) sees it at once ...
    assert lines["reloaded"].split() == want(new)                # ... and bofi_reload_env brings it in
    assert lines["unset"].split() == want(None)
    assert lines["generations"] == "2"                           # every reload bumps the generation of the graph keys


# ---- (b) the sources as text
def _sources():
    files = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    assert len(files) > 20
    return {os.path.basename(f): open(f).read() for f in files}


def test_getenv_only_in_the_reader():
    assert [f for f, text in _sources().items() if "getenv(" in text] == ["knobs.hip"]


def test_the_reload_generation_is_declared_once():
    src = _sources()
    decls = sorted((f, line.strip().startswith("extern")) for f, text in src.items() for line in re.findall(r"^.*\bint g_env_generation\b.*$", text, re.M))
    assert decls == [("bofi_knobs.h", True), ("knobs.hip", False)]                # one declaration, one definition
    assert not [f for f, text in src.items() if "BOFI_ENV_INT" in text or "env_seen" in text]


def test_every_name_is_a_row_and_every_row_is_read():
    src, rows = _sources(), _table_rows()
    literals = {(f, m.group(1)) for f, text in src.items() for m in re.finditer(r'"(BOFI_[A-Z0-9_]+)"', text)}
    assert all(name in rows for _, name in literals), sorted(literals)        # (the table's rows are identifiers: the reader makes the strings, so today there is none)
    for name in rows:
        users = [f for f, text in src.items() if f != "bofi_knobs.h" and re.search(r"\bknob(_set|_str|_live|_value)?\(" + name + r"\)", text)]
        assert users, f"{name} is a row that nothing reads"
