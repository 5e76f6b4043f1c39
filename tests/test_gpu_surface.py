"""The surface of evaluated captions on the MI355X (boficap_amd/csrc/surface.hip): ``bofi_caption_trim`` and ``bofi_sentence_lookup`` against the
host restatements of boficap_amd.surface (which tests/test_surface.py holds to the reference's own strings), and ``eval_split`` with
``remove_bad_endings`` / ``surface_stats`` on the tiny synthetic model.  Integers throughout: every comparison is exact."""
import json
import os

import numpy as np
import pytest
import torch

from test_cider import synthetic_corpus, write_df_pickle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -77
LANG_KEYS = ["Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L", "CIDEr", "entropy", "perplexity"]
DIV_KEYS = ["Div-1", "Div-2", "mBLEU_1", "mBLEU_2", "mBLEU_3", "mBLEU_4", "self_cider"]
ORACLE_KEYS = [f"{a}_{k}" for a in ("oracle", "avg") for k in LANG_KEYS[:6]]
SURFACE_KEYS = ["novel_sentences", "vocab_size", "bad_count_rate"]


def crafted_rows(S):
    """The fixture's rows at width S: cut, or padded with 0."""
    with open(os.path.join(ROOT, "tests", "golden", "surface_text.json")) as f:
        rows = np.array(json.load(f)["rows"], dtype=np.int64)
    out = np.zeros((len(rows), S), dtype=np.int64)
    out[:, :min(S, rows.shape[1])] = rows[:, :S]
    return out


def word_sets(V):
    """(trim ids, count ids): five trim words, with the ids at the bit tables' word boundaries (31, 32, V - 1) in the sets."""
    return sorted({1, 6, 13, 31, V - 1}), sorted({1, 5, 9, 31, 32, V - 1})


def trim_rows(rows, S, V, seed):
    """``rows`` rows of S ids: the crafted rows first (as many as fit), then random rows over 12 ids of which 5 are trim words -- tails of 0 from a random
    position on most rows, none on the others -- and the ids -1, V and 2^31 planted in three of them."""
    rng = np.random.default_rng(seed)
    trim, _ = word_sets(V)
    pool = np.array(trim + [4, 5, 7, 8, 9, 14, 32 if V > 33 else 10], dtype=np.int64)
    assert len(set(pool.tolist())) == 12
    seq = pool[rng.integers(0, 12, (rows, S))]
    for row in seq:
        if rng.integers(0, 4) > 0:
            row[int(rng.integers(0, S + 1)):] = 0
    crafted = crafted_rows(S)[:max(0, rows - 1)]
    seq[:len(crafted)] = crafted
    if rows >= 5:
        for r, v in zip((rows - 1, rows - 2, rows - 3), (-1, V, 2 ** 31)):
            seq[r, int(rng.integers(0, S))] = v
    return seq


def launch_trim(seq, limit, trim_bits, count_bits, V, pad, in_place):
    """bofi_caption_trim through the C ABI on buffers over-allocated with a sentinel: (out_seq, out_len, out_bad) as host arrays, tails checked."""
    from boficap_amd import hip
    rows, S = seq.shape
    flat = torch.full((rows * S + 64,), SENTINEL, dtype=torch.int64, device="cuda")
    src = torch.from_numpy(seq).cuda().contiguous()
    if in_place:
        flat[:rows * S] = src.reshape(-1)
        src = flat
    length = torch.full((rows + 16,), SENTINEL, dtype=torch.int32, device="cuda")
    bad = torch.full((rows + 16,), SENTINEL, dtype=torch.int32, device="cuda")
    hip.check(hip.lib().bofi_caption_trim(hip.ptr(src), rows, S, limit, hip.ptr(trim_bits), hip.ptr(count_bits), V, pad, hip.ptr(flat), hip.ptr(length), hip.ptr(bad),
                                          hip.stream_ptr()), "bofi_caption_trim")
    flat, length, bad = flat.cpu().numpy(), length.cpu().numpy(), bad.cpu().numpy()
    assert (flat[rows * S:] == SENTINEL).all() and (length[rows:] == SENTINEL).all() and (bad[rows:] == SENTINEL).all()
    if not in_place:
        assert np.array_equal(src.cpu().numpy(), seq)                            # the input stays as it was
    return flat[:rows * S].reshape(rows, S), length[:rows], bad[:rows]


def device_bits(ids, V):
    from boficap_amd.surface import bit_table
    return torch.from_numpy(bit_table(ids, V).view(np.int32)).cuda()


@pytest.mark.parametrize("S", [1, 20, 64])
def test_caption_trim_equals_the_host_restatement(S):
    from boficap_amd.surface import trim_host
    seen_long_run = seen_all_bad = False
    for V in (33, 9495):
        trim, count = word_sets(V)
        tb, cb = device_bits(trim, V), device_bits(count, V)
        for rows in (1, 5, 257):                                                 # 257: a partial last workgroup, rows that do not divide by four
            seq = trim_rows(rows, S, V, seed=1000 * S + rows + V)
            for limit in (0, 3, -2):                                             # (-2: the id -1 stands inside a caption and must not be looked up)
                for k, (t_ids, c_ids, t_dev, c_dev) in enumerate(((trim, count, tb, cb), (None, count, None, cb), (trim, None, tb, None))):
                    want = trim_host(seq, t_ids, c_ids, limit, pad=0)
                    in_place = (k + rows + limit) % 2 == 0
                    got = launch_trim(seq, limit, t_dev, c_dev, V, 0, in_place)
                    for name, g, w in zip(("out_seq", "out_len", "out_bad"), got, want):
                        assert np.array_equal(g, w), (name, S, V, rows, limit, k, in_place)
                    if k == 0 and limit == 0:
                        plain = trim_host(seq, None, None, limit)[1]
                        seen_long_run |= bool(((plain - want[1]) >= 3).any())
                        all_bad = [n >= 2 and all(v in trim for v in r[:n]) for r, n in zip(seq.tolist(), plain.tolist())]
                        assert all(kept == n for bad_row, kept, n in zip(all_bad, want[1].tolist(), plain.tolist()) if bad_row)       # left as they are
                        seen_all_bad |= any(all_bad)
                # both ways on the same rows, and another pad
                a = launch_trim(seq, 0, tb, cb, V, 0, True)
                b = launch_trim(seq, 0, tb, cb, V, 0, False)
                assert all(np.array_equal(x, y) for x, y in zip(a, b))
                padded = launch_trim(seq, 0, tb, cb, V, -5, False)
                assert np.array_equal(padded[0], trim_host(seq, trim, count, 0, pad=-5)[0])
    if S >= 20:
        assert seen_long_run and seen_all_bad                                    # the random rows reach both: runs of three and more, captions of trim words alone


def test_caption_surface_trims_in_one_launch_and_checks_its_arguments():
    from boficap_amd import hip
    from boficap_amd.surface import CaptionSurface, trim_host
    V = 9495
    trim, count = word_sets(V)
    surface = CaptionSurface(V, trim, count, "cuda")
    seq = trim_rows(257, 20, V, seed=5)
    dev = torch.from_numpy(seq).cuda()
    out, length, bad = surface.trim(dev)
    assert out.is_cuda and out.dtype == torch.int64 and length.dtype == torch.int32 and bad.dtype == torch.int32
    want = trim_host(seq, trim, count)
    assert np.array_equal(out.cpu().numpy(), want[0]) and np.array_equal(length.cpu().numpy(), want[1]) and np.array_equal(bad.cpu().numpy(), want[2])
    assert np.array_equal(dev.cpu().numpy(), seq)                                # not modified unless asked
    assert surface.bad_count_rate(bad) == float(int(want[2].sum())) / 257 and 0.0 < surface.bad_count_rate(bad) < 1.0
    kept = surface.trim(dev, remove=False)
    plain = trim_host(seq, None, count)
    assert np.array_equal(kept[0].cpu().numpy(), plain[0]) and np.array_equal(kept[2].cpu().numpy(), plain[2])
    again = surface.trim(out, remove=False)                                      # a trimmed row is its own canonical form
    assert torch.equal(again[0], out) and torch.equal(again[1], length) and torch.equal(again[2], bad)
    same = surface.trim(dev, in_place=True)[0]
    assert same.data_ptr() == dev.data_ptr() and np.array_equal(dev.cpu().numpy(), want[0])
    host_in = surface.trim(crafted_rows(20).astype(np.int32))                    # host ids of another integer type
    assert np.array_equal(host_in[0].cpu().numpy(), trim_host(crafted_rows(20), trim, count)[0])
    with pytest.raises(ValueError):
        surface.trim(torch.zeros(3, 65, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        surface.trim(torch.from_numpy(seq), in_place=True)
    lib = hip.lib()
    buf, small = torch.zeros(64, dtype=torch.int64, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
    for rows, S, Vx in ((1, 0, 10), (1, 65, 10), (-1, 8, 10), (1, 8, 0)):
        assert lib.bofi_caption_trim(hip.ptr(buf), rows, S, 0, None, None, Vx, 0, hip.ptr(buf), hip.ptr(small), hip.ptr(small), hip.stream_ptr()) == 1
    assert b"caption_trim" in lib.bofi_last_error()
    assert lib.bofi_caption_trim(None, 1, 8, 0, None, None, 10, 0, hip.ptr(buf), hip.ptr(small), hip.ptr(small), hip.stream_ptr()) == 1
    assert lib.bofi_caption_trim(hip.ptr(buf), 0, 8, 0, None, None, 10, 0, hip.ptr(buf), hip.ptr(small), hip.ptr(small), hip.stream_ptr()) == 0
    assert lib.bofi_sentence_lookup(hip.ptr(buf), hip.ptr(small), 1, 8, None, 1, 8, 10, hip.ptr(small), hip.ptr(small), hip.stream_ptr()) == 1
    assert b"sentence_lookup" in lib.bofi_last_error()
    assert lib.bofi_sentence_lookup(hip.ptr(buf), hip.ptr(small), 1, 8, None, 0, 65, 10, hip.ptr(small), hip.ptr(small), hip.stream_ptr()) == 1
    torch.cuda.synchronize()


def training_rows(M, St, S, with_empty, seed):
    """M distinct canonical rows of width St over the ids 1..6 -- some longer than S when St > S -- with, as far as M allows, the empty row (when asked), [7]
    (the highest row) and [1] (the lowest non-empty one) among them: the first and the last row are short enough for any S."""
    rng = np.random.default_rng(seed)
    if M == 0:
        return np.zeros((0, St), dtype=np.int64)
    fixed = ([[0] * St] if with_empty else []) + [[7] + [0] * (St - 1), [1] + [0] * (St - 1)]
    rows = {tuple(r) for r in fixed[:M]}
    while len(rows) < M:
        n = int(rng.integers(1, St + 1))
        rows.add(tuple(rng.integers(1, 7, n).tolist() + [0] * (St - n)))
    return np.array(sorted(rows), dtype=np.int64)


def query_rows(train, S, V, seed):
    """Rows of S ids with their lengths: every training row that fits (hits, the first and the last among them), strict prefixes, extensions, random rows,
    the empty row, rows longer than the training width, ids outside the vocabulary, and a row whose length stops short of its ids."""
    rng = np.random.default_rng(seed)
    lists = [[]]
    for row in train.tolist():
        ids = [v for v in row if v != 0]
        if len(ids) <= S:
            lists.append(ids)
            if len(ids) >= 2:
                lists.append(ids[:int(rng.integers(1, len(ids)))])               # a strict prefix
            if len(ids) < S:
                lists.append(ids + [int(rng.integers(1, 7))])                    # an extension
    for _ in range(40):
        lists.append(rng.integers(1, 8, int(rng.integers(1, S + 1))).tolist())
    lists += [[7], [1], [6] * S, [1] * S, [V, 2, 2 ** 31], [3, V + 7], [2 ** 31], [3, -1, 2]]
    seq, length = np.zeros((len(lists) + 1, S), dtype=np.int64), np.zeros(len(lists) + 1, dtype=np.int32)
    for r, ids in enumerate(lists):
        seq[r, :len(ids)], length[r] = ids, len(ids)
    seq[-1, :3], length[-1] = [3, 2, 5], 2                                       # the length says what is kept
    return seq, length


@pytest.mark.parametrize("M", [0, 1, 2, 1000])
def test_sentence_lookup_equals_the_host_restatement(M):
    from boficap_amd import hip
    from boficap_amd.surface import TrainSentences, lookup_host
    S, V = 12, 33
    for St in (S - 4, S, S + 4):
        for with_empty in (False, True):
            rows = training_rows(M, St, S, with_empty, seed=7 * M + St)
            shuffled = np.concatenate([rows, rows[:3]])[np.random.default_rng(M).permutation(len(rows) + min(3, len(rows)))] if M else rows
            train = TrainSentences(shuffled, "cuda")                             # duplicates and order are the class's business
            assert train.M == M and train.St == St and np.array_equal(train.host, rows.astype(np.int32)) and train.rows.dtype == torch.int32
            seq, length = query_rows(rows, S, V, seed=M + St)
            want_novel, want_seen = lookup_host(seq, length, rows, V)
            n = len(seq)
            novel = torch.full((n + 16,), SENTINEL, dtype=torch.int32, device="cuda")
            seen = torch.zeros(V + 16, dtype=torch.int32, device="cuda")
            seen[V:] = SENTINEL
            seq_dev, length_dev = torch.from_numpy(seq).cuda(), torch.from_numpy(length).cuda()      # (named: they must outlive the launch)
            hip.check(hip.lib().bofi_sentence_lookup(hip.ptr(seq_dev), hip.ptr(length_dev), n, S,
                                                     hip.ptr(train.rows if M else None), M, St, V, hip.ptr(novel), hip.ptr(seen), hip.stream_ptr()), "bofi_sentence_lookup")
            novel, seen = novel.cpu().numpy(), seen.cpu().numpy()
            assert (novel[n:] == SENTINEL).all() and (seen[V:] == SENTINEL).all()
            assert np.array_equal(novel[:n], want_novel), (M, St, with_empty, np.flatnonzero(novel[:n] != want_novel))
            assert np.array_equal(seen[:V], want_seen)
            assert set(np.flatnonzero(seen[:V]).tolist()) == {v for row, k in zip(seq.tolist(), length.tolist()) for v in row[:k] if 0 <= v < V}
            assert novel[0] == (0 if with_empty and M else 1)                    # the empty row: a sentence like any other
            if M >= 2:
                first, last = ([v for v in rows[i].tolist() if v] for i in (0, M - 1))
                hits = {tuple(r[:k]): int(f) for r, k, f in zip(seq.tolist(), length.tolist(), novel[:n].tolist())}
                assert hits[tuple(first)] == 0 and hits[tuple(last)] == 0 and last == [7]
            if M:
                assert 0 < int(novel[:n].sum()) < n


def test_sentence_stats_equal_the_host_restatement():
    from boficap_amd.surface import CaptionSurface, TrainSentences, sentence_stats, sentence_stats_host
    V, S = 33, 12
    rows = training_rows(1000, S + 4, S, True, seed=3)
    train = TrainSentences(rows, "cuda")
    seq, length = query_rows(rows[::3], S, V, seed=11)
    seq, length = np.concatenate([seq, seq[::2], seq[:5]]), np.concatenate([length, length[::2], length[:5]])      # duplicates among the generated rows
    canon, kept, _ = CaptionSurface(V, None, None, "cuda", limit=0).trim(np.where(np.arange(S)[None, :] < length[:, None], seq, 0))
    want = sentence_stats_host(canon.cpu().numpy(), kept.cpu().numpy(), rows, V)
    got = sentence_stats(canon, kept, train, V)
    assert got == want and list(got) == ["novel_sentences", "vocab_size"] and 0.0 < got["novel_sentences"] < 1.0 and got["vocab_size"] >= 7
    assert sentence_stats(canon, kept, TrainSentences(np.zeros((0, 5), dtype=np.int64), "cuda"), V)["novel_sentences"] == len(np.unique(canon.cpu().numpy(), axis=0)) / len(seq)


def rows_of(entries, S):
    rows = np.zeros((len(entries), S), dtype=np.int64)
    for j, p in enumerate(entries):
        rows[j, :len(p["seq"])] = p["seq"]
    return rows


def pick_word_sets(first):
    """From the first run's captions: a trim id some captions end with -- so that at least one shortens and at least one does not -- and count ids that
    flag some of the trimmed captions and not others."""
    from boficap_amd.surface import trim_host
    plain = trim_host(first)[1]
    ends = [int(r[n - 1]) for r, n in zip(first, plain) if n > 0]
    for b in sorted(set(ends), key=lambda v: (-ends.count(v), v)):
        kept = trim_host(first, [b])[1]
        if (kept < plain).any() and (kept == plain).any():
            trimmed = trim_host(first, [b])
            after = [int(r[n - 1]) for r, n in zip(trimmed[0], trimmed[1]) if n > 0]
            count = [b, max(set(after), key=lambda v: (after.count(v), -v))]
            return [b], count
    raise AssertionError(f"no final id of {ends} splits the captions into shortened and untouched ones")


def model_and_feats(mode, labels, weight_cache, manifest):
    """NAIC: the tiny model of tests/test_gpu_lang_eval.py on the labels' images.  SAIC: with those weights the greedy semi-autoregressive decode emits nothing, so
    the weights of the tiny_saic_multi fixture (several phrases per caption; pinned to the reference by tests/golden/tiny_saic_multi.npz) and, for the first six
    images, that fixture's features."""
    from conftest import load_golden
    from test_gpu_lang_eval import tiny_model
    if mode == "NAIC":
        return tiny_model(), labels.feats
    import captioning.models as models
    m = manifest["tiny_saic_multi"]
    cfg, sd = weight_cache(m["config"], m["seed"], m["gen_scale"], m["digest"], m.get("patch"))
    opt = cfg.to_opt()
    opt.bofi_compute_dtype, opt.bofi_max_batch = torch.float32, 64
    model = models.setup(opt)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return model.cuda(), np.concatenate([load_golden("tiny_saic_multi")["att_feats"], labels.feats[6:]])


@pytest.mark.parametrize("mode", ["NAIC", "SAIC"])
def test_eval_split_trims_before_it_scores_and_reports_the_surface(mode, tmp_path, weight_cache, manifest):
    from boficap_amd import eval_utils
    from boficap_amd.config import TINY
    from boficap_amd.surface import CaptionSurface, TrainSentences, sentence_stats_host, trim_host
    S, N, V = TINY.seq_length, 16, TINY.tgt_vocab
    df = str(tmp_path / "tiny-idxs.p")
    write_df_pickle(df, synthetic_corpus(200, seed=4, vocab=64, lengths=(3, 20)))
    labels = eval_utils.SyntheticLabels(TINY, N, 5, seed=3)
    model, feats = model_and_feats(mode, labels, weight_cache, manifest)
    base = {"batch_size": 4, "language_eval": 1, "inference_mode": mode, "verbose_loss": 0}
    kw0 = dict(base)
    _, p0, s0 = eval_utils.eval_split(model, feats, labels, kw0)
    assert list(s0) == LANG_KEYS
    ev = kw0["lang_eval"]
    first = rows_of(p0, S)
    trim, count = pick_word_sets(first)
    want_seq, want_len, want_bad = trim_host(first, trim, count)
    plain_len = trim_host(first)[1]
    assert (want_len < plain_len).any() and (want_len == plain_len).any()         # the trim is no no-op, and not everything is trimmed
    surface = CaptionSurface(V, trim, count, "cuda")

    # the options name what they miss, before anything is decoded
    with pytest.raises(ValueError, match="caption_surface.*vocab"):
        eval_utils.eval_split(model, feats, labels, dict(base, remove_bad_endings=1))
    with pytest.raises(ValueError, match="train_sentences"):
        eval_utils.eval_split(model, feats, labels, dict(base, surface_stats=1, sample_n=3, caption_surface=surface, cached_tokens=df))

    kw1 = dict(base, lang_eval=ev, remove_bad_endings=1, caption_surface=surface)
    _, p1, s1 = eval_utils.eval_split(model, feats, labels, kw1)
    assert [p["seq"] for p in p1] == [r[:n].tolist() for r, n in zip(want_seq, want_len)]
    assert list(s1) == LANG_KEYS and set(p1[0]) == set(p0[0])
    assert {k: s1[k] for k in LANG_KEYS[:6]} == ev.evaluate(want_seq)             # the scorers read the trimmed ids
    assert {k: s0[k] for k in LANG_KEYS[:6]} == ev.evaluate(first)                # ... as the first run's read the untrimmed ones
    assert s1["entropy"] == s0["entropy"] and s1["perplexity"] == s0["perplexity"]
    for a, b in zip(p0, p1):                                                     # what describes the decode stays
        assert all(a[k] == b[k] for k in ("image_id", "phrase_num", "phrase_length", "entropy", "perplexity"))

    # bad_count_rate alone: nothing is trimmed, the flags are those of the captions as they stand
    kw2 = dict(base, lang_eval=ev, surface_stats=1, caption_surface=surface)
    _, p2, s2 = eval_utils.eval_split(model, feats, labels, kw2)
    assert [p["seq"] for p in p2] == [p["seq"] for p in p0] and list(s2) == LANG_KEYS + ["bad_count_rate"]
    assert {k: s2[k] for k in LANG_KEYS} == s0
    assert s2["bad_count_rate"] == float(int(trim_host(first, None, count)[2].sum())) / N and s2["bad_count_rate"] > 0.0

    # sampled captions: a first pass gives the training sentences (half of its captions), a second pass from the same seed is looked up in them
    model._sample_calls = 0
    kw3 = dict(base, lang_eval=ev, remove_bad_endings=1, caption_surface=surface, sample_n=3, cached_tokens=df, eval_oracle=1)
    _, _, s3 = eval_utils.eval_split(model, feats, labels, kw3)
    assert list(s3) == LANG_KEYS + DIV_KEYS + ORACLE_KEYS
    sampled = rows_of(kw3["preds_n"], S)
    assert np.array_equal(trim_host(sampled, trim, count)[0], sampled)           # the stored samples are trimmed: trimming them again changes nothing
    train = TrainSentences(sampled[::2], "cuda")
    model._sample_calls = 0
    kw4 = dict(kw3, surface_stats=1, train_sentences=train, diversity_eval=kw3["diversity_eval"])
    _, p4, s4 = eval_utils.eval_split(model, feats, labels, kw4)
    assert [p["seq"] for p in kw4["preds_n"]] == [p["seq"] for p in kw3["preds_n"]] and [p["seq"] for p in p4] == [p["seq"] for p in p1]
    assert list(s4) == LANG_KEYS + DIV_KEYS + ORACLE_KEYS + SURFACE_KEYS             # the new keys come last
    assert {k: s4[k] for k in s3} == s3
    want = sentence_stats_host(sampled, [len(p["seq"]) for p in kw4["preds_n"]], train.host, V)
    assert s4["novel_sentences"] == want["novel_sentences"] and s4["vocab_size"] == want["vocab_size"] and isinstance(s4["vocab_size"], int)
    assert s4["novel_sentences"] <= 0.5 + 1e-12 and s4["vocab_size"] >= 1        # every other sample is a training sentence
    assert s4["bad_count_rate"] == float(int(want_bad.sum())) / N
    # outside language_eval: the sampled captions' statistics alone, after the diversity keys
    model._sample_calls = 0
    kw5 = {"batch_size": 4, "inference_mode": mode, "verbose_loss": 0, "sample_n": 3, "cached_tokens": df, "diversity_eval": kw3["diversity_eval"],
           "remove_bad_endings": 1, "surface_stats": 1, "caption_surface": surface, "train_sentences": train}
    s5 = eval_utils.eval_split(model, feats, labels, kw5)[2]
    assert list(s5) == DIV_KEYS + SURFACE_KEYS[:2] and s5["novel_sentences"] == s4["novel_sentences"] and s5["vocab_size"] == s4["vocab_size"]

    if mode == "NAIC":
        # the surface built from a vocabulary, captions, and the regions of the kept words only
        vocab = dict(TINY.to_opt().vocab)
        vocab[str(trim[0])] = "the"                                              # in both of the reference's word lists
        kw6 = dict(base, lang_eval=ev, remove_bad_endings=1, surface_stats=1, vocab=vocab, attn_topk=2)
        _, p6, s6 = eval_utils.eval_split(model, feats, labels, kw6)
        only = trim_host(first, trim, trim)
        assert [p["seq"] for p in p6] == [r[:n].tolist() for r, n in zip(only[0], only[1])]
        assert [len(p["regions"]) for p in p6] == only[1].tolist() and all(len(w) <= 2 for p in p6 for w in p["regions"])
        assert [p["caption"] for p in p6] == [" ".join(vocab.get(str(v), "UNK") for v in p["seq"] if v > 6) for p in p6]
        assert kw6["caption_surface"].trim_ids == trim and kw6["caption_surface"].count_ids == trim
        assert list(s6) == LANG_KEYS + ["bad_count_rate"] and s6["bad_count_rate"] == float(int(only[2].sum())) / N
        kw7 = dict(base, lang_eval=ev, vocab=vocab, attn_topk=2)                 # the same run with the options off: untouched
        _, p7, s7 = eval_utils.eval_split(model, feats, labels, kw7)
        assert [p["seq"] for p in p7] == [p["seq"] for p in p0] and list(s7) == LANG_KEYS and "caption_surface" not in kw7
        assert {k: s7[k] for k in LANG_KEYS[:6]} == {k: s0[k] for k in LANG_KEYS[:6]}
        assert [len(p["regions"]) for p in p7] == plain_len.tolist()


def test_tools_eval_trims_and_prints_the_surface_statistics(tmp_path):
    """tools/eval.py --remove_bad_endings 1 --surface_stats 1 --bad_endings W in a fresh process against eval_split here, on the same model, features, label
    file and image list."""
    import pickle
    import re
    import subprocess
    import sys
    from boficap_amd import eval_utils, weights as W
    from boficap_amd.collate import synthetic_captions
    from boficap_amd.config import TINY
    from boficap_amd.data import LabelStore
    from boficap_amd.surface import CaptionSurface, TrainSentences, trim_host
    from test_gpu_lang_eval import tiny_model
    S, n_img, per = TINY.seq_length, 8, 5
    labels, plen, psyn = synthetic_captions(TINY, n_img * per, seed=21)
    arrays = {"labels": labels[:, 1:S + 1].astype(np.uint32), "label_start_ix": (np.arange(n_img) * per + 1).astype(np.uint32),
              "label_end_ix": ((np.arange(n_img) + 1) * per).astype(np.uint32), "label_length": (labels[:, 1:S + 1] > 0).sum(1).astype(np.uint32),
              "phrase_num": (plen > 0).sum(1).astype(np.uint32), "phrase_length": plen.astype(np.uint32), "phrase_label": psyn.astype(np.uint32)}
    df, npz, pth, pkl, dump, js = (str(tmp_path / f) for f in ("tiny-idxs.p", "labels.npz", "model.pth", "infos.pkl", "out.json", "images.json"))
    np.savez(npz, **arrays)
    write_df_pickle(df, synthetic_corpus(200, seed=4, vocab=64, lengths=(3, 20)))
    torch.save({k: torch.from_numpy(v) for k, v in W.make_state_dict(TINY, seed=0, gen_scale=6.0).items()}, pth)
    splits = ["val", "val", "test", "train", "train", "train", "restval", "restval"]
    with open(js, "w") as f:
        json.dump({"images": [{"id": 100 + i, "split": s} for i, s in enumerate(splits)]}, f)
    train_ixs = [i for i, s in enumerate(splits) if s not in ("val", "test")]
    feats = W.synthetic_att_feats(n_img, 36, TINY.att_feat_size, seed=1235)      # tools/eval.py's --synthetic images
    store = LabelStore(arrays, pad_idx=TINY.pad_idx, bos_idx=TINY.bos_idx, eos_idx=TINY.eos_idx, len_idx=TINY.len_idx)
    opt = TINY.to_opt()
    base = {"batch_size": 4, "seq_per_img": per, "language_eval": 1, "cached_tokens": df}
    _, p0, _ = eval_utils.eval_split(tiny_model(max_batch=4).eval(), feats, store, dict(base))
    trim, count = pick_word_sets(rows_of(p0, S))
    vocab = dict(opt.vocab)
    vocab[str(count[1])] = "the"                                                 # one of the reference's counted words; the trimmed word goes by --bad_endings
    with open(pkl, "wb") as f:
        pickle.dump({"opt": opt, "vocab": vocab}, f, protocol=2)
    cmd = [sys.executable, os.path.join(ROOT, "tools", "eval.py"), "--model", pth, "--infos_path", pkl, "--synthetic", str(n_img), "--batch_size", "4", "--dtype", "f32",
           "--input_label_npz", npz, "--input_json", js, "--cached_tokens", df, "--dump_json", dump, "--language_eval", "1", "--sample_n", "3",
           "--remove_bad_endings", "1", "--surface_stats", "1", "--bad_endings", vocab[str(trim[0])]]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    surface = CaptionSurface(TINY.tgt_vocab, trim, [count[1]], "cuda")
    kw = dict(base, vocab=vocab, sample_n=3, remove_bad_endings=1, surface_stats=1, caption_surface=surface, train_sentences=TrainSentences.from_store(store, train_ixs, "cuda"))
    _, predictions, stats = eval_utils.eval_split(tiny_model(max_batch=4).eval(), feats, store, kw)
    assert list(stats)[-3:] == SURFACE_KEYS
    want = trim_host(rows_of(p0, S), trim, [count[1]])
    assert [p["seq"] for p in predictions] == [r[:n].tolist() for r, n in zip(want[0], want[1])] and stats["bad_count_rate"] == float(int(want[2].sum())) / n_img
    printed = dict(re.findall(r"(\w+) (-?[0-9.]+|nan)", out.stdout.split("surface statistics ")[1].splitlines()[0]))
    assert list(printed) == SURFACE_KEYS and printed == {k: f"{stats[k]:.6f}" for k in SURFACE_KEYS}
    with open(dump) as f:
        dumped = json.load(f)
    assert set(dumped) == {"predictions", "preds_n", "lang_stats"} and list(dumped["lang_stats"])[-3:] == SURFACE_KEYS
    assert [dumped["lang_stats"][k] for k in SURFACE_KEYS] == [stats[k] for k in SURFACE_KEYS]
    assert [p["seq"] for p in dumped["predictions"]] == [p["seq"] for p in predictions]
    assert [p["caption"] for p in dumped["predictions"]] == [p["caption"] for p in predictions]
    assert [p["seq"] for p in dumped["preds_n"]] == [p["seq"] for p in kw["preds_n"]]
    printed_lang = dict(re.findall(r"(\w+) (-?[0-9.]+|nan)", out.stdout.split("language scores ")[1].splitlines()[0]))
    assert printed_lang["CIDEr"] == f"{stats['CIDEr']:.6f}" and printed_lang["Bleu_1"] == f"{stats['Bleu_1']:.6f}"
