"""The validation pass: ``LanguageEval`` against the three scorers called on their own, ``eval_split`` against per-batch ``mode='sample'`` calls and
the loss pass tools/eval.py ran before it moved into boficap_amd.eval_utils, the validation loop of tools/train.py and ``tools/eval.py
--language_eval 1``."""
import json
import os
import pickle
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_rouge import eval_ids, rouge_of

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANG_KEYS = ["Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L", "CIDEr", "entropy", "perplexity"]


def corpus(seed, images=48, refs=5, S=16):
    """References (rows, 0-padded) and decoded rows with inner 0s, with no 0 at all, and one that starts with a 0."""
    rng = np.random.default_rng(seed)
    gts = []
    for _ in range(images):
        g = rng.integers(1, 13, (refs, 18))
        for row in g:
            row[int(rng.integers(2, 19)):] = 0
        gts.append(g)
    seq = rng.integers(1, 13, (images, S))
    for j, row in enumerate(seq):
        if j % 3 == 0:
            row[int(rng.integers(1, S)):] = 0                  # ids, then padding
        elif j % 3 == 1:
            row[int(rng.integers(1, S - 1))] = 0               # an inner 0: what follows it is not read
    seq[7] = np.arange(1, S + 1) % 12 + 1                      # no 0 at all: the whole row
    seq[8, 0] = 0                                              # an empty caption
    return gts, seq


def alone(gts, seq):
    """The three scorers on their own, on the 'eval' token lists as id strings."""
    from boficap_amd.bleu import Bleu
    from boficap_amd.cider import CiderD
    strs = lambda rows: [" ".join(map(str, eval_ids(r))) for r in rows]
    g = {i: strs(rows) for i, rows in enumerate(gts)}
    r = {i: strs([seq[i]]) for i in range(len(gts))}
    bleu, _ = Bleu(4, device="cuda").compute_score(g, r)
    cider, _ = CiderD("corpus", device="cuda").compute_score(g, [{"image_id": i, "caption": r[i]} for i in range(len(gts))])
    rouge = float(np.mean(np.array([rouge_of(eval_ids(seq[i]), [eval_ids(x) for x in gts[i]])[0] for i in range(len(gts))])))
    return bleu, cider, rouge


def test_language_eval_equals_the_scorers_on_their_own():
    from boficap_amd.lang_eval import LanguageEval
    gts, seq = corpus(1)
    ev = LanguageEval(gts, "cuda")
    ent, ppl = torch.arange(48, dtype=torch.float32).cuda(), np.linspace(1.0, 2.0, 48).astype(np.float32)
    stats = ev.evaluate(torch.from_numpy(seq).cuda(), ent, ppl)
    assert list(stats) == LANG_KEYS
    bleu, cider, rouge = alone(gts, seq)
    print(f"CIDEr {stats['CIDEr']!r} / {cider!r}, ROUGE_L {stats['ROUGE_L']!r} / {rouge!r}, BLEU {[stats[f'Bleu_{k}'] for k in range(1, 5)]}")
    assert [stats[f"Bleu_{k}"] for k in range(1, 5)] == bleu                     # the same counts through the same host arithmetic: bit-equal
    assert abs(stats["CIDEr"] - cider) <= 1e-15
    assert abs(stats["ROUGE_L"] - rouge) <= 1e-15
    assert stats["entropy"] == 23.5 and abs(stats["perplexity"] - float(np.mean(ppl.astype(np.float64)))) == 0.0
    assert 0.0 < stats["Bleu_4"] < stats["Bleu_1"] < 1.0 and stats["CIDEr"] > 0.0 and 0.0 < stats["ROUGE_L"] < 1.0
    # a second evaluation on the kept records, other candidates, ids from the host: a fresh object's result; and as id strings
    _, seq2 = corpus(2)
    again = ev.evaluate(seq2)
    assert list(again) == LANG_KEYS[:6]
    assert again == LanguageEval(gts, "cuda").evaluate(seq2) and again != {k: stats[k] for k in again}
    as_strings = [[" ".join(map(str, eval_ids(r))) for r in g] for g in gts]
    assert again == LanguageEval(as_strings, "cuda").evaluate(torch.from_numpy(seq2).cuda().to(torch.int32))
    bleu2, cider2, rouge2 = alone(gts, seq2)
    assert [again[f"Bleu_{k}"] for k in range(1, 5)] == bleu2 and abs(again["CIDEr"] - cider2) <= 1e-15 and abs(again["ROUGE_L"] - rouge2) <= 1e-15
    with pytest.raises(ValueError):
        ev.evaluate(seq2[:5])


def tiny_model(max_batch=64):
    import captioning.models as models
    from boficap_amd import weights as W
    from boficap_amd.config import TINY
    opt = TINY.to_opt()
    opt.bofi_compute_dtype, opt.bofi_max_batch = torch.float32, max_batch
    model = models.setup(opt)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in W.make_state_dict(TINY, seed=0, gen_scale=6.0).items()}, strict=True)
    return model.cuda()


def loss_pass_before_the_move(model, feats, store, batch_size, seq_per_img):
    """The loop tools/eval.py ran in its own body before it became eval_utils.validation_loss."""
    from boficap_amd.loss_wrapper import LanguageModelCriterion_UIC
    crit, rng, loss_sum, loss_evals = LanguageModelCriterion_UIC(), np.random.default_rng(0), 0.0, 0
    with torch.no_grad():
        for i in range(0, len(feats), batch_size):
            att = torch.from_numpy(np.ascontiguousarray(feats[i:i + batch_size])).cuda()
            fc = torch.zeros(att.size(0), 0, device="cuda")
            hb = store.batch(range(i, i + att.size(0)), seq_per_img, rng)
            hb.pop("gts", None)
            b = {k: torch.from_numpy(v).cuda() for k, v in hb.items()}
            outs = model(fc, att.float(), b["labels"], None, b["phrase_num"], b["phrase_length"], b["phrase_syn"],
                         b["extend_phrase_syn_seq"], b["extend_phrase_seq"], b["extend_phrase_seq_mask"])
            loss_sum += float(crit(*outs, b["phrase_num"], b["phrase_length"], b["phrase_syn"], b["labels"])[0])
            loss_evals += 1
    return loss_sum / max(1, loss_evals)


def test_eval_split_on_the_tiny_model():
    from boficap_amd import eval_utils
    from boficap_amd.config import TINY
    model = tiny_model()
    labels = eval_utils.SyntheticLabels(TINY, 8, 5, seed=3)
    feats = labels.feats
    model.eval()
    want_loss = loss_pass_before_the_move(model, feats, labels, 4, 5)
    want = {}
    with torch.no_grad():
        for mode in ("NAIC", "SAIC"):
            rows = []
            for i in (0, 4):
                att = torch.from_numpy(feats[i:i + 4]).cuda()
                seq = model(torch.zeros(4, 0, device="cuda"), att, None, opt={"train_mode": mode, "sample_method": "greedy", "sample_n": 1}, mode="sample")[0]
                rows.extend([int(v) for v in r if v > 0] for r in seq.cpu().tolist())
            want[mode] = rows
    model.train()
    kw = {"batch_size": 4, "seq_per_img": 5, "language_eval": 1, "lang_eval": None}
    for mode in ("NAIC", "SAIC"):
        kws = dict(kw, inference_mode=mode)
        val_loss, predictions, lang_stats = eval_utils.eval_split(model, feats, labels, kws)
        kw["lang_eval"] = kws["lang_eval"]                                       # the caller keeps the references' records
        assert model.training
        assert [p["seq"] for p in predictions] == want[mode] and [p["image_id"] for p in predictions] == list(range(8))
        assert all(set(p) == {"image_id", "seq", "phrase_num", "phrase_length", "entropy", "perplexity"} for p in predictions)
        assert val_loss == want_loss and val_loss > 0
        assert list(lang_stats) == LANG_KEYS
    assert kw["lang_eval"] is not None and kw["lang_eval"].images == 8
    # the references alone: no loss, the same captions and scores
    gts = [labels.gts(i) for i in range(8)]
    val_loss, p2, s2 = eval_utils.eval_split(model, feats, gts, {"batch_size": 4, "language_eval": 1, "inference_mode": "SAIC"})
    assert val_loss == 0.0 and [p["seq"] for p in p2] == want["SAIC"] and [s2[k] for k in LANG_KEYS[:6]] == [lang_stats[k] for k in LANG_KEYS[:6]]
    assert eval_utils.eval_split(model, feats, None, {"batch_size": 4, "inference_mode": "SAIC"})[2] is None


def test_training_validates_and_keeps_the_best_checkpoint(tmp_path):
    """python tools/train.py with a validation pass every 2 of 4 iterations, in a fresh process."""
    from boficap_amd.checkpoint import load_infos
    ck = str(tmp_path / "ck")
    cmd = [sys.executable, os.path.join(ROOT, "tools", "train.py"), "--tiny", "--no_graph", "--max_iters", "4", "--save_checkpoint_every", "2",
           "--val_images_use", "8", "--language_eval", "1", "--checkpoint_path", ck]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "iter 2 validation loss" in out.stdout and "iter 4 validation loss" in out.stdout and " SA_CIDEr " in out.stdout
    assert os.path.exists(os.path.join(ck, "model-best.pth")) and os.path.exists(os.path.join(ck, "infos_bofi-best.pkl"))
    assert not os.path.exists(os.path.join(ck, "model-2.pth"))                   # (--save_history_ckpt is off)
    infos, hist = load_infos(ck, "bofi")
    val = hist["val_result_history"]
    assert sorted(val) == [2, 4]
    for it in (2, 4):
        assert set(val[it]) == {"loss", "lang_stats", "predictions"}
        assert list(val[it]["lang_stats"]) == LANG_KEYS and len(val[it]["predictions"]) == 8 and val[it]["loss"] > 0
    assert infos["best_val_score"] == max(val[2]["lang_stats"]["CIDEr"], val[4]["lang_stats"]["CIDEr"])
    best_infos, _ = load_infos(ck, "bofi", "best")
    best_it = 2 if val[2]["lang_stats"]["CIDEr"] >= val[4]["lang_stats"]["CIDEr"] else 4
    assert best_infos["iter"] == best_it and best_infos["best_val_score"] == infos["best_val_score"]


def test_tools_eval_prints_the_scores_of_eval_split(tmp_path):
    """tools/eval.py --language_eval 1 in a fresh process against eval_split here, on the same model, features and label file."""
    from boficap_amd import eval_utils, weights as W
    from boficap_amd.collate import synthetic_captions
    from boficap_amd.config import TINY
    from boficap_amd.data import LabelStore
    S, n_img, per = TINY.seq_length, 8, 5
    labels, plen, psyn = synthetic_captions(TINY, n_img * per, seed=21)
    arrays = {"labels": labels[:, 1:S + 1].astype(np.uint32), "label_start_ix": (np.arange(n_img) * per + 1).astype(np.uint32),
              "label_end_ix": ((np.arange(n_img) + 1) * per).astype(np.uint32), "label_length": (labels[:, 1:S + 1] > 0).sum(1).astype(np.uint32),
              "phrase_num": (plen > 0).sum(1).astype(np.uint32), "phrase_length": plen.astype(np.uint32), "phrase_label": psyn.astype(np.uint32)}
    npz, pth, pkl, dump = (str(tmp_path / n) for n in ("labels.npz", "model.pth", "infos.pkl", "out.json"))
    np.savez(npz, **arrays)
    torch.save({k: torch.from_numpy(v) for k, v in W.make_state_dict(TINY, seed=0, gen_scale=6.0).items()}, pth)
    opt = TINY.to_opt()
    with open(pkl, "wb") as f:
        pickle.dump({"opt": opt, "vocab": opt.vocab}, f, protocol=2)
    cmd = [sys.executable, os.path.join(ROOT, "tools", "eval.py"), "--model", pth, "--infos_path", pkl, "--synthetic", str(n_img), "--batch_size", "4",
           "--dtype", "f32", "--input_label_npz", npz, "--dump_json", dump]
    out = subprocess.run(cmd + ["--language_eval", "1"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    model = tiny_model(max_batch=4)
    feats = W.synthetic_att_feats(n_img, 36, TINY.att_feat_size, seed=1235)      # tools/eval.py's --synthetic images
    store = LabelStore(arrays, pad_idx=TINY.pad_idx, bos_idx=TINY.bos_idx, eos_idx=TINY.eos_idx, len_idx=TINY.len_idx)
    val_loss, predictions, stats = eval_utils.eval_split(model.eval(), feats, store, {"batch_size": 4, "seq_per_img": per, "language_eval": 1, "vocab": opt.vocab})
    printed = dict(re.findall(r"(\w+) (-?[0-9.]+|nan)", out.stdout.split("language scores ")[1].splitlines()[0]))
    assert printed["CIDEr"] == f"{stats['CIDEr']:.6f}" and printed["ROUGE_L"] == f"{stats['ROUGE_L']:.6f}" and printed["Bleu_4"] == f"{stats['Bleu_4']:.6f}"
    assert f"validation loss {val_loss:.4f} over 2 batches" in out.stdout
    with open(dump) as f:
        dumped = json.load(f)
    assert set(dumped) == {"predictions", "lang_stats"} and dumped["lang_stats"]["CIDEr"] == stats["CIDEr"]
    assert [p["seq"] for p in dumped["predictions"]] == [p["seq"] for p in predictions]
    assert dumped["predictions"][0]["caption"] == predictions[0]["caption"]
    # without the flag the dump stays the list it was
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    with open(dump) as f:
        plain = json.load(f)
    assert isinstance(plain, list) and [p["seq"] for p in plain] == [p["seq"] for p in predictions] and "language scores" not in out.stdout
