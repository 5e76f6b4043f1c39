"""The surface of evaluated captions, host side: ``surface.trim_host`` against what the reference's ``decode_sequence`` / ``count_bad`` returned
(tests/golden/surface_text.json, written by dev/make_surface_golden.py), the word sets' id tables, the canonical training sentences and the
lookup's restatement, the declaration of the two entry points, and the argument errors of tools/eval.py.  tests/test_gpu_surface.py holds the
device side against the same restatements."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "surface_text.json")) as f:
        return json.load(f)


def test_trim_host_reproduces_the_reference_strings_and_flags():
    from boficap_amd.surface import COUNT_WORDS, TRIM_WORDS, ids_of, trim_host
    fx = fixture()
    vocab, rows = fx["vocab"], np.array(fx["rows"], dtype=np.int64)
    word_id = {w: int(k) for k, w in vocab.items()}
    assert len(word_id) == len(vocab)                                            # the strings map back to ids one to one
    trim_ids, count_ids = ids_of(vocab, TRIM_WORDS), ids_of(vocab, COUNT_WORDS)
    assert len(fx["cases"]) == 4 and {(c["remove_bad_endings"], c["limit"]) for c in fx["cases"]} == {(0, 0), (0, 3), (1, 0), (1, 3)}
    shortened = 0
    for case in fx["cases"]:
        limit = case["limit"]
        out, length, bad = trim_host(rows, trim_ids if case["remove_bad_endings"] else None, count_ids, limit)
        for r, caption in enumerate(case["captions"]):
            want = [word_id[w] for w in caption.split(" ") if w]
            assert out[r].tolist() == want + [0] * (rows.shape[1] - len(want)), (case["remove_bad_endings"], limit, fx["what"][r])
            assert int(length[r]) == len(want)
        assert bad.tolist() == case["bad"], (case["remove_bad_endings"], limit)
        plain = trim_host(rows, None, None, limit)
        shortened += int((length < plain[1]).sum())
        assert plain[2].tolist() == [0] * len(rows)                              # no count set: no flag
    assert shortened >= 10
    # the quirks of the reference's loop, in its own words
    by_row = {tuple(r): i for i, r in enumerate(fx["rows"])}
    trimmed = next(c for c in fx["cases"] if c["remove_bad_endings"] == 1 and c["limit"] == 0)["captions"]
    assert trimmed[by_row[(1, 2, 1, 0, 0, 0, 0, 0)]] == "a the a" and trimmed[by_row[(1, 0, 0, 0, 0, 0, 0, 0)]] == "a"
    assert trimmed[by_row[(4, 1, 2, 6, 3, 1, 2, 0)]] == "man" and trimmed[by_row[(0, 0, 0, 0, 0, 0, 0, 0)]] == ""
    # another pad, and ids no table holds
    out, length, bad = trim_host([[4, 1, 0, 9]], trim_ids, count_ids, 0, pad=-7)
    assert out.tolist() == [[4, -7, -7, -7]] and length.tolist() == [1] and bad.tolist() == [0]
    out, length, bad = trim_host([[2 ** 31, 1, -1, 4]], trim_ids, count_ids, -5)
    assert out.tolist() == [[2 ** 31, 1, -1, 4]] and length.tolist() == [4]
    out, length, bad = trim_host([[4, 2 ** 31, 1, 0]], trim_ids, count_ids, 0)
    assert out.tolist() == [[4, 2 ** 31, 0, 0]] and bad.tolist() == [0]


def test_word_sets_restate_the_reference_lists():
    from boficap_amd.surface import COUNT_WORDS, TRIM_WORDS
    assert len(TRIM_WORDS) == 14 and len(COUNT_WORDS) == 17                      # misc.py:17-18 and eval_utils.py:28-29 without their doubled 'the'
    assert TRIM_WORDS - COUNT_WORDS == {"this", "his", "her", "that"}
    assert COUNT_WORDS - TRIM_WORDS == {"before", "after", "upon", "near", "is", "are", "am"}


def test_ids_of_and_bit_table():
    from boficap_amd.surface import bit_table, ids_of
    V = 70
    vocab = {str(i): f"w{i}" for i in range(1, V)}
    vocab.update({"31": "a", "32": "the", str(V - 1): "of", "5": "a", "40": "zebra"})      # 'a' twice: two ids of one word
    ids = ids_of(vocab, ["a", "the", "of", "absent", "a"])
    assert ids == [5, 31, 32, V - 1]
    t = bit_table(ids, V)
    assert t.dtype == np.uint32 and t.shape == (3,)
    assert t.tolist() == [(1 << 5) | (1 << 31), 1 << 0, 1 << ((V - 1) & 31)]
    member = [(int(t[i >> 5]) >> (i & 31)) & 1 for i in range(V)]
    assert [i for i in range(V) if member[i]] == ids
    assert bit_table([], 33).tolist() == [0, 0] and bit_table([32, 32, 0], 33).tolist() == [1, 1]
    assert bit_table([31], 32).shape == (1,)
    for bad in ([V], [-1]):
        with pytest.raises(ValueError):
            bit_table(bad, V)
    assert ids_of(vocab, []) == [] and ids_of({}, ["a"]) == []


def test_training_sentences_are_canonical_distinct_and_sorted():
    from boficap_amd.surface import TrainSentences, canonical_rows
    rows = np.array([[5, 6, 0, 9], [5, 6, 0, 0], [2, 0, 0, 0], [0, 7, 7, 7], [5, 6, 7, 8], [5, 0, 0, 0], [12, 1, 0, 0], [0, 0, 0, 0]], dtype=np.uint32)
    canon = canonical_rows(rows)
    assert canon.tolist() == [[5, 6, 0, 0], [5, 6, 0, 0], [2, 0, 0, 0], [0, 0, 0, 0], [5, 6, 7, 8], [5, 0, 0, 0], [12, 1, 0, 0], [0, 0, 0, 0]]
    assert canonical_rows(rows, limit=5)[[0, 4, 6]].tolist() == [[0, 0, 0, 0], [0, 0, 0, 0], [12, 0, 0, 0]]
    train = TrainSentences(rows, "cpu")                                          # (the host side of the class: no launch is involved)
    uniq = train.host
    assert uniq.dtype == np.int32 and (train.M, train.St) == (6, 4) and train.rows.dtype.is_floating_point is False and train.rows.tolist() == uniq.tolist()
    assert uniq.tolist() == [[0, 0, 0, 0], [2, 0, 0, 0], [5, 0, 0, 0], [5, 6, 0, 0], [5, 6, 7, 8], [12, 1, 0, 0]]
    assert [tuple(r) for r in uniq.tolist()] == sorted(set(tuple(r) for r in canon.tolist()))      # distinct, lexicographic by row
    empty = TrainSentences(np.zeros((0, 7), dtype=np.int64), "cpu")
    assert (empty.M, empty.St) == (0, 7) and empty.host.shape == (0, 7)
    for bad in (np.zeros((3, 65), dtype=np.int64), np.zeros(5, dtype=np.int64), np.array([[2 ** 31, 0]])):
        with pytest.raises(ValueError):
            TrainSentences(bad, "cpu")


def test_lookup_host_on_prefixes_extensions_and_widths():
    from boficap_amd.surface import lookup_host
    train = np.array([[0, 0, 0, 0], [5, 6, 0, 0], [5, 6, 7, 8], [9, 0, 0, 0]])
    seq = np.array([[5, 6, 0, 0], [5, 0, 0, 0], [5, 6, 7, 0], [5, 6, 7, 8], [0, 0, 0, 0], [9, 0, 0, 0], [9, 3, 0, 0], [70, 0, 0, 0]])
    length = np.array([2, 1, 3, 4, 0, 1, 2, 1])
    novel, seen = lookup_host(seq, length, train, 64)
    assert novel.tolist() == [0, 1, 1, 0, 0, 0, 1, 1]                            # a strict prefix and an extension are novel; the empty row is a sentence
    assert np.flatnonzero(seen).tolist() == [3, 5, 6, 7, 8, 9]                   # id 70 is outside the vocabulary: skipped
    assert lookup_host(seq, length, train[1:], 64)[0].tolist() == [0, 1, 1, 0, 1, 0, 1, 1]      # ... absent from the table: novel
    # S != St: zero extension on either side; a row longer than St is novel
    wide = np.concatenate([seq, np.zeros((len(seq), 2), dtype=np.int64)], axis=1)
    assert lookup_host(wide, length, train, 64)[0].tolist() == novel.tolist()
    assert lookup_host(seq, length, np.concatenate([train, np.zeros((4, 3), dtype=np.int64)], axis=1), 64)[0].tolist() == novel.tolist()
    assert lookup_host(seq, length, train[:, :2], 64)[0].tolist() == [0, 1, 1, 1, 0, 0, 1, 1]   # [5, 6, 7, 8] cut at 2 is [5, 6]: the 4-id row no longer matches
    # the lengths, not the ids past them, say what is kept
    assert lookup_host([[5, 6, 7, 8]], [2], train, 64)[0].tolist() == [0]
    # M = 0
    novel0, seen0 = lookup_host(seq, length, np.zeros((0, 4), dtype=np.int64), 64)
    assert novel0.tolist() == [1] * 8 and seen0.tolist() == seen.tolist()


def test_sentence_stats_count_duplicates_once_over_all_rows():
    from boficap_amd.surface import sentence_stats_host
    train = np.array([[5, 6, 0, 0], [9, 0, 0, 0]])
    seq = np.array([[5, 6, 0, 0], [7, 8, 0, 0], [7, 8, 0, 0], [7, 8, 0, 0], [9, 0, 0, 0], [4, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0]])
    length = np.array([2, 2, 2, 2, 1, 1, 0, 0])
    stats = sentence_stats_host(seq, length, train, 16)
    assert stats == {"novel_sentences": 3 / 8, "vocab_size": 6}                  # novel: (7 8), (4), (): once each; over the 8 rows before unique
    assert list(stats) == ["novel_sentences", "vocab_size"] and isinstance(stats["vocab_size"], int)
    # the reference's arithmetic on the same captions as strings (eval_utils.py:61-69)
    strings = [" ".join(str(v) for v in row[:n]) for row, n in zip(seq.tolist(), length.tolist())]
    training = {"5 6", "9"}
    generated = set(strings)
    assert stats["novel_sentences"] == float(len(generated - training)) / len(strings)
    assert stats["vocab_size"] == len({w for s in generated for w in s.split()})
    with pytest.raises(ValueError):
        sentence_stats_host(np.zeros((0, 4)), [], train, 16)


def test_header_and_ctypes_table_declare_the_entry_points_alike():
    from boficap_amd import build, hip
    header = open(os.path.join(ROOT, "include", "boficap_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, arity in (("bofi_caption_trim", 12), ("bofi_sentence_lookup", 11)):
        found = re.findall(r"\bint\s+" + name + r"\s*\(([^;{]*?)\)\s*;", code, flags=re.S)
        assert len(found) == 1 and found[0].count(",") + 1 == len(hip.SIGNATURES[name][1]) == arity, name
        assert found[0].rstrip().endswith("void* stream")
    assert "surface.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "surface.hip"))
    assert hip.ABI_VERSION == 5


def run_eval(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval.py"), *args], capture_output=True, text=True, timeout=120)


def test_tools_eval_refuses_the_options_without_what_they_need():
    out = run_eval("--remove_bad_endings", "1")
    assert out.returncode == 2 and "--infos_path" in out.stderr and "--bad_endings" in out.stderr
    out = run_eval("--surface_stats", "1", "--language_eval", "1", "--input_label_npz", "labels.npz")
    assert out.returncode == 2 and "--infos_path" in out.stderr and "--bad_endings" in out.stderr
    for extra in ([], ["--input_label_npz", "labels.npz"], ["--input_json", "images.json"]):
        out = run_eval("--surface_stats", "1", "--sample_n", "2", "--bad_endings", "a,the", *extra)
        assert out.returncode == 2 and "--input_label_npz" in out.stderr and "--input_json" in out.stderr, out.stderr[-500:]
