"""The evaluation of a split as the reference's ``eval_split`` runs it for a UIC model (captioning/utils/eval_utils.py:425-520): the validation
loss, one greedy caption per image, and the language scores that need no Java (boficap_amd.lang_eval).

    val_loss, predictions, lang_stats = eval_split(model, feats, store_or_gts, eval_kwargs)
    val_loss, predictions, lang_stats = eval_split(model, feats, store_or_gts, eval_kwargs, sample_n=5)       # + eval_kwargs['preds_n']

``feats``: region features [N, R, F] (array or tensor on the host), or a REGION SOURCE -- an object with ``__len__`` and ``ragged(i0, i1)`` -> a
``features.RaggedBatch`` of images i0 .. i1 - 1 (``features.RegionSource``: per-image feature files of 10..100 regions): every batch is then staged ragged
and padded to its longest image on the device, with the loader's mask (None when the batch's images have equal counts).  A source built with a box store
(the loader's use_box: ``RegionSource(store, ids, box_store=..., sizes=...)``) hands over ``BoxRaggedBatch``es -- geometry columns, area sort and the padded
width come from the same launch; such a model is decode-only, so ``verbose_loss`` must be 0.  ``store_or_gts``: a label source with ``batch(image_ixs, seq_per_img, rng)``
and ``gts(ix)`` (``data.LabelStore``, ``SyntheticLabels``) -- the loss is computed and the references come from it --, or the per-image
references alone (integer rows or id strings; no loss then), or None.  ``eval_kwargs``:

    inference_mode   'NAIC' (default; the batches go through ``model.decode_many``) or 'SAIC' (one ``mode='sample'`` call per batch)
    batch_size       images per batch (default 64);  seq_per_img  captions per image of the loss pass (default 5)
    language_eval    1: ``lang_stats`` from ``eval_kwargs['lang_eval']``, a ``LanguageEval`` of these images' references that the CALLER keeps
                     from one validation to the next (built here, and stored under that key, if absent)
    image_ixs        the label source's image of every row of ``feats`` (default 0 .. N - 1)
    verbose_loss     0: no loss pass;  vocab  {str(id): word} for the entries' 'caption'
    batches_per_launch, in_flight, fused_vocab     ``decode_many``'s knobs
    refine_rounds, refine_method     NAIC only: extra filling passes as ``decode_many`` takes them ('feed_back', the default, or 'mask_predict'); with
                     'mask_predict' the pass that emitted each token is stored under ``eval_kwargs['refine_round']`` (int32 [N, S]), and entropy /
                     perplexity come from the emitting passes' statistics
    attn_topk        K in 1..8, NAIC only: every entry gains 'regions', one list per id of its 'seq': the [region, weight] pairs of the K image regions the word's
                     position attended to most (mean over heads of the last decoder layer's cross-attention in the filling pass), heaviest first
    sample_n         N > 1 (or the ``sample_n`` argument): after the greedy pass, N captions per image are drawn through ``mode='sample'`` with
                     ``sample_method='sample'`` (eval_split_n, eval_utils.py:670-700, ``sample_n_method='sample'``); their entries are stored under
                     ``eval_kwargs['preds_n']``, and ``lang_stats`` gains the diversity statistics of boficap_amd.diversity ('Div-1', 'Div-2',
                     'mBLEU_1'..'mBLEU_4', 'self_cider'; per image under ``eval_kwargs['diversity_per_image']``) on the document frequencies of
    sample_n_method  'sample' (default) or 'nbest' (the reference's 'bs', the N best of a beam, for the non-autoregressive decode -- where it is exact and no search):
                     the ``sample_n`` rows per image are the N most probable captions of the filling pass, most probable first (``mode='sample'`` with
                     ``opt['nbest']``: one decode plus two small launches; deterministic, where 'sample' draws).  N <= 8, inference_mode 'NAIC' only, not with mask-predict or
                     ``require_words``; ``suppress_UNK`` / ``ban_words`` apply to the list too, ``decoding_constraint`` / ``block_trigrams`` stay refused.  Every
                     entry of ``preds_n`` carries 'logp' (float64 sum of its positions' log-probs; -inf for the empty rows of an image that has fewer than N
                     distinct captions); the number of such images is ``lang_stats['nbest_short']``.  The rows feed the diversity statistics, the oracle scores
                     and the surface statistics exactly as sampled rows do
    nbest_no_repeat  1, with ``sample_n_method`` 'nbest' and ``sample_n`` <= 6 (a ValueError otherwise): the rows are the ``sample_n`` most probable captions with no
                     adjacent repeated word (ids >= 7), exactly -- ``opt['nbest_no_repeat']``, bofi_vocab_nbest_norepeat.  The greedy predictions stay the plain decode's;
                     ``decoding_constraint`` with the list stays refused.  Keys as above
    sample_n_method 'diverse'   the reference's 'dbs' (diverse beam search, one beam per group, Hamming diversity at the same position) for the non-autoregressive
                     decode, where it is exact and no search: the ``sample_n`` rows per image are a set decoded group after group, group g the exact maximiser of its
                     log-prob minus ``diversity_lambda`` (the reference's key and default, 0.5) times the number of earlier groups with the same word at the same
                     position (``opt['diverse']``, bofi_vocab_diverse: one decode plus two small launches; deterministic).  Row 0 is the greedy caption.
                     ``diverse_no_repeat`` 1: every caption of the set is free of adjacent repeated words (ids >= 7) and ``sample_n`` <= 6; else ``sample_n`` <= 8.
                     Refusals and banned words as with 'nbest'; entries carry 'logp' (the caption's own log-prob); ``lang_stats['diverse_short']`` counts the images
                     with fewer than ``sample_n`` captions (degenerate rows, or no repeat-free caption)
    cached_tokens    a df pickle of scripts/prepro_ngrams.py: a path, or a name resolved as data/<name>.p (default 'coco-train-idxs')
    eval_oracle      1, with ``language_eval`` 1 and ``sample_n`` > 1 (nothing changes otherwise): every sampled caption is scored against its image's
                     references and ``lang_stats`` gains 'oracle_<M>' (the best of an image's N, averaged over the images) and 'avg_<M>' (their mean)
                     for M = Bleu_1..Bleu_4, ROUGE_L, CIDEr (``LanguageEval.evaluate_n``); per image under ``eval_kwargs['oracle_per_image']``
    remove_bad_endings   1: every caption loses its trailing function words (decode_sequence under REMOVE_BAD_ENDINGS, boficap_amd.surface) before the entries are
                     built and before any scorer reads it -- the greedy ids before ``LanguageEval.evaluate``, the sampled ids before ``preds_n``, the diversity
                     statistics and the oracle scores: 'seq', 'caption' and 'regions' cover the kept ids only.  'phrase_num', 'phrase_length', entropy, perplexity
                     and ``eval_kwargs['refine_round']`` describe the decode and stay.  ``model(..., mode='sample')`` itself returns untrimmed ids
    surface_stats    1: with ``language_eval`` 1 ``lang_stats`` gains 'bad_count_rate' (the share of captions that end in a word of surface.COUNT_WORDS), and with
                     ``sample_n`` > 1 'novel_sentences' and 'vocab_size' of the sampled captions against ``eval_kwargs['train_sentences']``, a
                     ``surface.TrainSentences`` (required then); the new keys follow every other key, in the order novel_sentences, vocab_size, bad_count_rate
    caption_surface  the ``surface.CaptionSurface`` both options use, kept by the caller; built from ``vocab`` (and stored under this key) if absent
"""
from __future__ import annotations

import numpy as np
import torch

from . import weights as W
from .collate import synthetic_training_batch

LANG_KEYS = ("Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L", "CIDEr", "entropy", "perplexity")


def entry_of(i, k, seq, pn, pl, ent, ppl, vocab=None):
    """The prediction entry of row ``k`` of a decoded batch whose first image is ``i``."""
    ids = [int(v) for v in seq[k].tolist() if v > 0]
    entry = {"image_id": i + k, "seq": ids, "phrase_num": int(pn[k]), "phrase_length": [int(v) for v in pl[k].tolist() if v > 0],
             "entropy": float(ent[k]), "perplexity": float(ppl[k])}
    if vocab:
        entry["caption"] = " ".join(vocab.get(str(v), "UNK") for v in ids if v > 6)
    return entry


def regions_of(seq_row, top_row, top_w_row):
    """The 'regions' field of a prediction entry: for every emitted word -- every position of ``seq_row`` [S] whose id is > 0, the ids of the entry's 'seq' -- the
    [region, weight] pairs of ``top_row`` / ``top_w_row`` [S, K] (``decode_many(attn_topk=K)``), heaviest first; index -1 marks an empty slot and is skipped."""
    return [[[int(r), float(w)] for r, w in zip(top_row[t].tolist(), top_w_row[t].tolist()) if r >= 0] for t, v in enumerate(seq_row.tolist()) if v > 0]


def with_regions(entry, r, k):
    """``entry`` with the 'regions' of row ``k`` of a decoded batch ``r`` that carries attn_top / attn_top_w (unchanged otherwise)."""
    if "attn_top" in r:
        entry["regions"] = regions_of(r["seq"][k], r["attn_top"][k], r["attn_top_w"][k])
    return entry


def is_region_source(feats) -> bool:
    return hasattr(feats, "ragged") and hasattr(feats, "__len__")


def device_batch(source, i0: int, i1: int, dtype=torch.float32):
    """Images i0 .. i1 - 1 of a region source on the device as the loader's collate hands them over: (att_feats [b, longest, F] in ``dtype``, att_masks
    float32 [b, longest] or None)."""
    from .features import att_masks_of
    att, att_len = source.ragged(i0, min(i1, len(source))).to_device(out_dtype=dtype)
    return att, att_masks_of(att_len, att.size(1))


def validation_loss(model, feats, store, batch_size: int, seq_per_img: int, image_ixs=None):
    """The loss of eval_split (verbose_loss, eval_utils.py:440-453) as a pass of its own: (sum of the batches' LanguageModelCriterion_UIC losses,
    number of batches).  Image i of ``feats`` is image ``image_ixs[i]`` (default i) of ``store``."""
    from .loss_wrapper import LanguageModelCriterion_UIC
    if model.cfg.att_feat_padded != model.cfg.att_feat_size:
        raise NotImplementedError(f"the validation loss runs mode='forward', which is not built for att_feat_size = {model.cfg.att_feat_size} (box features "
                                  "are decode-only): pass verbose_loss = 0")
    crit, rng, loss_sum, loss_evals = LanguageModelCriterion_UIC(), np.random.default_rng(0), 0.0, 0
    with torch.no_grad():
        for i in range(0, len(feats), batch_size):
            if is_region_source(feats):
                att, masks = device_batch(feats, i, i + batch_size)
            else:
                att, masks = torch.from_numpy(np.ascontiguousarray(feats[i:i + batch_size])).cuda(), None
            fc = torch.zeros(att.size(0), 0, device="cuda")
            ixs = range(i, i + att.size(0)) if image_ixs is None else [int(x) for x in image_ixs[i:i + att.size(0)]]
            hb = store.batch(ixs, seq_per_img, rng)
            hb.pop("gts", None)
            b = {k: torch.from_numpy(v).cuda() for k, v in hb.items()}
            outs = model(fc, att.float(), b["labels"], masks, b["phrase_num"], b["phrase_length"], b["phrase_syn"],
                         b["extend_phrase_syn_seq"], b["extend_phrase_seq"], b["extend_phrase_seq_mask"])
            loss_sum += float(crit(*outs, b["phrase_num"], b["phrase_length"], b["phrase_syn"], b["labels"])[0])
            loss_evals += 1
    return loss_sum, loss_evals


class SyntheticLabels:
    """A label source for the synthetic stream: ``n_img`` images of ``seq_per_img`` synthetic captions each from a fixed seed, and the region
    features that go with them; the captions are the images' references."""

    def __init__(self, cfg, n_img: int, seq_per_img: int, seed: int = 0, regions: int = 36):
        self.num_images, self.seq_per_img = int(n_img), int(seq_per_img)
        self.host = synthetic_training_batch(cfg, self.num_images, self.seq_per_img, seed=seed)
        self.feats = W.synthetic_att_feats(self.num_images, regions, cfg.att_feat_size, seed=seed)

    def batch(self, image_ixs, seq_per_img: int, rng=None):
        if int(seq_per_img) != self.seq_per_img:
            raise ValueError(f"the synthetic labels hold {self.seq_per_img} captions per image, not {seq_per_img}")
        ixs = np.asarray(list(image_ixs), dtype=np.int64)
        return {k: np.ascontiguousarray(v[ixs]) for k, v in self.host.items()}

    def gts(self, ix: int):
        return self.host["labels"][int(ix), :, 1:-1]


SAMPLE_N_METHODS = ("sample", "nbest", "diverse")


def sample_n_method_of(eval_kwargs, mode: str = "NAIC", sample_n: int = 1) -> str:
    """``eval_kwargs['sample_n_method']``: 'sample' (the default), 'nbest' or 'diverse'; any other string is a ValueError that names them.  With ``sample_n`` > 1, 'nbest'
    and 'diverse' are a ValueError where the rows cannot be made: SAIC mode, more than 8 captions per image, mask-predict, ``decoding_constraint`` /
    ``block_trigrams`` (``diverse_options_of`` has the set's own keys)."""
    method = eval_kwargs.get("sample_n_method", "sample") or "sample"
    if method not in SAMPLE_N_METHODS:
        raise ValueError(f"sample_n_method {method!r}: 'sample' (sample_n random draws) and 'nbest' (the sample_n most probable captions of the filling pass) are served, "
                         "and 'diverse' (a Hamming-diverse set of sample_n captions of the filling pass)")
    if method == "diverse" and int(sample_n) > 1:
        from .hip import DIVERSE_MAX
        if mode != "NAIC":
            raise ValueError("sample_n_method 'diverse' decodes the non-autoregressive filling pass's rows group by group: inference_mode 'NAIC' only")
        if int(sample_n) > DIVERSE_MAX:
            raise ValueError(f"sample_n_method 'diverse': at most {DIVERSE_MAX} captions per image, got sample_n = {int(sample_n)}")
        if eval_kwargs.get("refine_method", "feed_back") == "mask_predict":
            raise ValueError("sample_n_method 'diverse': not with refine_method 'mask_predict' (kept positions do not hold their row's first id)")
        if int(eval_kwargs.get("decoding_constraint", 0)) == 1 or int(eval_kwargs.get("block_trigrams", 0) or 0) == 1:
            raise ValueError("sample_n_method 'diverse': not with decoding_constraint / block_trigrams (the set stands beside the plain decode; diverse_no_repeat = 1 "
                             "keeps adjacent repeats out of the set)")
    if method == "nbest" and int(sample_n) > 1:
        from .hip import NBEST_MAX
        if mode != "NAIC":
            raise ValueError("sample_n_method 'nbest' lists the non-autoregressive filling pass's captions: inference_mode 'NAIC' only")
        if int(sample_n) > NBEST_MAX:
            raise ValueError(f"sample_n_method 'nbest': at most {NBEST_MAX} captions per image, got sample_n = {int(sample_n)}")
        if eval_kwargs.get("refine_method", "feed_back") == "mask_predict":
            raise ValueError("sample_n_method 'nbest': not with refine_method 'mask_predict' (kept positions do not hold their row's first id)")
        if int(eval_kwargs.get("decoding_constraint", 0)) == 1 or int(eval_kwargs.get("block_trigrams", 0) or 0) == 1:
            raise ValueError("sample_n_method 'nbest': not with decoding_constraint / block_trigrams (a rule that couples neighbours needs per-last-id state: a "
                             "width-N list is no longer exact)")
    return method


def nbest_no_repeat_of(eval_kwargs, sample_n: int = 1) -> bool:
    """``eval_kwargs['nbest_no_repeat']`` (0, the default, or 1): the ``sample_n`` captions of ``sample_n_method='nbest'`` are the most probable ones with NO ADJACENT
    REPEATED WORD (bofi_vocab_nbest_norepeat, exact).  ValueError naming the key without ``sample_n_method='nbest'`` or with more than 6 captions per image.  (The
    constrained DECODE, ``decoding_constraint``, stays refused with the list: ``sample_n_method_of``.)"""
    if not int(eval_kwargs.get("nbest_no_repeat", 0) or 0):
        return False
    from .hip import NBEST_NR_MAX
    if (eval_kwargs.get("sample_n_method", "sample") or "sample") != "nbest":
        raise ValueError("nbest_no_repeat narrows the N-best list: it needs sample_n_method 'nbest'")
    if int(sample_n) > NBEST_NR_MAX:
        raise ValueError(f"nbest_no_repeat: at most {NBEST_NR_MAX} captions per image, got sample_n = {int(sample_n)}")
    return True


def diverse_options_of(eval_kwargs, sample_n: int = 1):
    """``eval_kwargs['diversity_lambda']`` (the reference's key and default, 0.5) and ``eval_kwargs['diverse_no_repeat']`` (0, the default, or 1) of
    ``sample_n_method='diverse'`` as (lambda, no_repeat).  ValueError naming the key: either key given without that method, a lambda that is negative, NaN or infinite,
    ``diverse_no_repeat`` outside {0, 1} or with more than 6 captions per image."""
    diverse = (eval_kwargs.get("sample_n_method", "sample") or "sample") == "diverse"
    nr = int(eval_kwargs.get("diverse_no_repeat", 0) or 0)
    lam = eval_kwargs.get("diversity_lambda")
    if not diverse:
        if nr:
            raise ValueError("diverse_no_repeat narrows the diverse set: it needs sample_n_method 'diverse'")
        return 0.5 if lam is None else float(lam), False         # (diversity_lambda without the method: the reference's files carry the key; it does nothing)
    lam = 0.5 if lam is None else float(lam)
    if not (lam >= 0.0) or lam == float("inf"):
        raise ValueError(f"diversity_lambda must be finite and >= 0, got {lam}")
    if nr not in (0, 1):
        raise ValueError(f"diverse_no_repeat is 0 or 1, got {nr}")
    from .hip import DIVERSE_NR_MAX
    if nr and int(sample_n) > DIVERSE_NR_MAX:
        raise ValueError(f"diverse_no_repeat: at most {DIVERSE_NR_MAX} captions per image, got sample_n = {int(sample_n)}")
    return lam, bool(nr)


def sample_n_predictions(model, feats, sample_n: int, mode: str = "NAIC", batch_size: int = 64, vocab=None, surface=None, method: str = "sample", ban_ids=None,
                         refine_rounds: int = 0, info=None, nbest_no_repeat: bool = False, diversity_lambda: float = 0.5,
                         diverse_no_repeat: bool = False):
    """eval_split_n (eval_utils.py:670-700): ``sample_n`` captions per image of ``feats`` through ``mode='sample'`` -- drawn (``method='sample'``, the reference's
    ``sample_n_method='sample'``) or the ``sample_n`` most probable captions of the NAIC filling pass, most probable first (``method='nbest'``: ``opt['nbest']``, under
    ``ban_ids`` and after ``refine_rounds`` feed-back rounds; rows past an image's count are the empty captions the kernel wrote).  Returns (entries {'image_id',
    'seq'[, 'caption'][, 'logp']} in row order, the ids [N * sample_n, S] on the device); an entry's 'seq' holds the ids before the first id <= 0 (decode_sequence);
    'logp' (``'nbest'`` only) is the caption's float64 total, -inf on an empty row past the count.  ``info``: a dict that receives 'nbest_short', the number of images
    with fewer than ``sample_n`` captions.  ``nbest_no_repeat`` (``'nbest'`` only, ``sample_n`` <= 6): the list is of the captions with no adjacent repeated word
    (``opt['nbest_no_repeat']``); an image may then have no caption at all (every row empty, every 'logp' -inf).  ``method='diverse'``: the Hamming-diverse set of
    ``sample_n`` captions (``opt['diverse']`` with ``diversity_lambda`` and ``diverse_no_repeat``: bofi_vocab_diverse), group 0 first, under ``ban_ids`` and after
    ``refine_rounds``; 'logp' is each caption's own log-prob and ``info`` receives 'diverse_short'.  ``surface``: a ``CaptionSurface`` -- the ids are trimmed of their bad endings on the device first, and both results are
    the trimmed ones."""
    if method not in SAMPLE_N_METHODS:
        raise ValueError(f"sample_n_method {method!r}: 'sample' and 'nbest' are served, and 'diverse'")
    if method == "nbest" and mode != "NAIC":
        raise ValueError("sample_n_method 'nbest' lists the non-autoregressive filling pass's captions: inference_mode 'NAIC' only")
    if method == "diverse" and mode != "NAIC":
        raise ValueError("sample_n_method 'diverse' decodes the non-autoregressive filling pass's rows group by group: inference_mode 'NAIC' only")
    n, ragged = int(sample_n), is_region_source(feats)
    host = feats if ragged else _torch_feats(feats)
    step = batch_size if mode == "NAIC" else max(1, min(batch_size, model.max_batch // n))       # the SAIC sampler decodes images x n rows
    rows, logps, short = [], [], 0
    with torch.no_grad():
        for i in range(0, len(host), step):
            if ragged:
                att, masks = device_batch(host, i, i + step)
            else:
                att, masks = host[i:i + step].cuda(), None
            if att.dtype != torch.float32 and att.dtype != model.compute_dtype:
                att = att.float()
            fc = torch.zeros(att.size(0), 0, device="cuda")
            if method == "nbest":
                opt = {"train_mode": mode, "sample_method": "greedy", "sample_n": 1, "nbest": n, "refine_rounds": int(refine_rounds), "ban_ids": list(ban_ids or ())}
                if nbest_no_repeat:
                    opt["nbest_no_repeat"] = 1
                model(fc, att, masks, opt=opt, mode="sample")
                nb = model.last_nbest
                rows.append(nb["seq"].reshape(-1, nb["seq"].size(-1)))
                logps.append(nb["logp"].reshape(-1))
                short += int((nb["count"] < n).sum())
            elif method == "diverse":
                opt = {"train_mode": mode, "sample_method": "greedy", "sample_n": 1, "diverse": n, "diversity_lambda": float(diversity_lambda),
                       "diverse_no_repeat": 1 if diverse_no_repeat else 0, "refine_rounds": int(refine_rounds), "ban_ids": list(ban_ids or ())}
                model(fc, att, masks, opt=opt, mode="sample")
                dv = model.last_diverse
                rows.append(dv["seq"].reshape(-1, dv["seq"].size(-1)))
                logps.append(dv["logp"].reshape(-1))
                short += int((dv["count"] < n).sum())
            else:
                rows.append(model(fc, att, masks, opt={"train_mode": mode, "sample_method": "sample", "sample_n": n}, mode="sample")[0])
    seq = torch.cat(rows)
    logp = torch.cat(logps).cpu().tolist() if logps else None
    if info is not None and method in ("nbest", "diverse"):
        info[method + "_short"] = short
    if surface is not None:
        seq = surface.trim(seq)[0]
    entries = []
    for j, row in enumerate(seq.cpu().tolist()):
        stop = next((q for q, v in enumerate(row) if v <= 0), len(row))
        entry = {"image_id": j // n, "seq": [int(v) for v in row[:stop]]}
        if vocab:
            entry["caption"] = " ".join(vocab.get(str(v), "UNK") for v in entry["seq"] if v > 6)
        if logp is not None:
            entry["logp"] = float(logp[j])
        entries.append(entry)
    return entries, seq


def diversity_stats(seq, sample_n: int, eval_kwargs):
    """The diversity statistics of sampled ids ``seq`` [N * sample_n, S] on the df file of ``eval_kwargs['cached_tokens']``; the
    ``DiversityEval`` is kept under ``eval_kwargs['diversity_eval']`` from one evaluation to the next.  Returns ({key: float}, per-image arrays)."""
    from .diversity import KEYS, DiversityEval
    ev = eval_kwargs.get("diversity_eval")
    if ev is None:
        ev = eval_kwargs["diversity_eval"] = DiversityEval(eval_kwargs.get("cached_tokens", "coco-train-idxs"), seq.device)
    out = ev.evaluate(seq, int(sample_n))
    return {k: out[k] for k in KEYS}, out["per_image"]


def constrained_rate(results) -> float:
    """Positions the constrained pick changed over positions emitted (the images' laid-out tokens), of ``decode_many``'s dicts."""
    changed = sum(int(r["constrained"].sum()) for r in results)
    emitted = sum(int(r["phrase_length"].sum()) for r in results)
    return changed / max(1, emitted)


def _torch_feats(feats):
    return feats if torch.is_tensor(feats) else torch.from_numpy(np.ascontiguousarray(feats))


def caption_surface(model, eval_kwargs):
    """The ``CaptionSurface`` of ``remove_bad_endings`` / ``surface_stats``: ``eval_kwargs['caption_surface']``, else one built from
    ``eval_kwargs['vocab']`` and kept under that key from one evaluation to the next."""
    surface = eval_kwargs.get("caption_surface")
    if surface is None:
        vocab = eval_kwargs.get("vocab")
        if not vocab:
            raise ValueError("remove_bad_endings / surface_stats need the ids of the bad-ending words: eval_kwargs['caption_surface'] (a "
                             "surface.CaptionSurface) or eval_kwargs['vocab'] ({str(id): word})")
        from .surface import CaptionSurface
        V = max(int(model.cfg.tgt_vocab), 1 + max(int(k) for k in vocab))
        surface = eval_kwargs["caption_surface"] = CaptionSurface.from_vocab(vocab, V, next(model.parameters()).device)
    return surface


def constraint_of(eval_kwargs, vocab, mode: str = "NAIC", sample_n: int = 1):
    """The constrained pick an evaluation asks for, as the keywords of ``TransformerModel.decode_many``: {} when ``suppress_UNK``, ``decoding_constraint`` (the
    reference's names; both default to 0 here: on this path the reference's options do nothing, and the defaults keep the captions) and ``ban_words`` (a list of
    words, or 'W1,W2,...') and ``block_trigrams`` (the reference's name and default, 0: no word trigram twice in a caption) are all off, else {'ban_ids': sorted ids,
    'no_repeat': bool}, with 'block_trigrams': True beside them when that option is on.  Words resolve to ids as the bad-ending words do (``surface.ids_of`` on
    ``vocab``; a word the vocabulary does not hold names no id).  ValueError where the options cannot apply: SAIC mode, ``fused_vocab``, mask-predict, sampling
    (``sample_n`` > 1) -- except that ``suppress_UNK`` / ``ban_words`` go with ``sample_n_method='nbest'`` and ``'diverse'``, whose rows are made under the same ban."""
    kw = eval_kwargs
    words = kw.get("ban_words") or []
    words = [w for w in words.split(",") if w] if isinstance(words, str) else list(words)
    unk, rep, tri = int(kw.get("suppress_UNK", 0)) == 1, int(kw.get("decoding_constraint", 0)) == 1, int(kw.get("block_trigrams", 0) or 0) == 1
    if not (unk or rep or words or tri):
        return {}
    if mode != "NAIC":
        raise ValueError("suppress_UNK / decoding_constraint / ban_words / block_trigrams constrain the non-autoregressive filling pass: inference_mode 'NAIC' only")
    if kw.get("fused_vocab", False):
        raise ValueError("suppress_UNK / decoding_constraint / ban_words / block_trigrams: not with fused_vocab (no distribution to re-pick from)")
    if kw.get("refine_method", "feed_back") == "mask_predict":
        raise ValueError("suppress_UNK / decoding_constraint / ban_words / block_trigrams: not with refine_method 'mask_predict'")
    listed = kw.get("sample_n_method", "sample") in ("nbest", "diverse")
    if int(sample_n) > 1 and (not listed or rep or tri):      # (banned ids go with the N-best list; a rule that couples neighbours does not)
        raise ValueError("suppress_UNK / decoding_constraint / ban_words / block_trigrams constrain greedy picks: not with sample_n > 1"
                         + (f" (sample_n_method {kw['sample_n_method']!r} takes suppress_UNK / ban_words only)" if listed else ""))
    if (unk or words) and not vocab:
        raise ValueError("suppress_UNK / ban_words need a vocabulary ({str(id): word})")
    from .surface import ids_of
    ids = ids_of(vocab, set(words) | ({"UNK"} if unk else set())) if (unk or words) else []
    if not ids and not rep and not tri:
        return {}                                                # (no such word in this vocabulary: nothing is banned and nothing launched)
    return dict({"ban_ids": ids, "no_repeat": rep}, **({"block_trigrams": True} if tri else {}))


def require_refusals(eval_kwargs, mode: str = "NAIC", sample_n: int = 1) -> None:
    """ValueError (naming ``require_words``) where required words cannot apply: SAIC mode, sampling, ``fused_vocab``, mask-predict, ``block_trigrams``."""
    kw = eval_kwargs
    if mode != "NAIC":
        raise ValueError("require_words place words on the non-autoregressive filling pass: inference_mode 'NAIC' only")
    if int(sample_n) > 1:
        raise ValueError("require_words place words on greedy picks: not with sample_n > 1")
    if kw.get("fused_vocab", False):
        raise ValueError("require_words: not with fused_vocab (no distribution to place the words by)")
    if kw.get("refine_method", "feed_back") == "mask_predict":
        raise ValueError("require_words: not with refine_method 'mask_predict'")
    if int(kw.get("block_trigrams", 0) or 0) == 1:
        raise ValueError("require_words: not with block_trigrams (a placement could create a blocked trigram)")


def required_of(eval_kwargs, vocab, keys, mode: str = "NAIC", sample_n: int = 1, ban_ids=()):
    """The required words an evaluation asks for (``eval_kwargs['require_words']``: a list of words -- or 'W1,W2,...' -- for every image, or a dict from image key to
    word list; ``keys``: the images' keys in order, matched as they are or as strings) as (ids, words): per image the id list ``decode_many(require_ids=...)`` takes
    and the words it stands for, duplicates dropped; None when no image requires a word.  Words resolve through ``vocab`` ({str(id): word}; the lowest id of a word):
    a word it does not hold is a ValueError that names it, as are more than 8 words for an image, a word that is also banned, and the options required words cannot
    go with (``require_refusals``).
    An item that contains a space is a PHRASE ('fire hydrant'): its words resolve one by one (an unknown one is the ValueError, naming that word), at most 4 of them --
    unless the vocabulary holds the whole item as one entry, which wins over splitting.  If any image has a phrase the whole evaluation goes through
    ``decode_many(require_phrases=...)``: every entry of ``ids`` is then a list of UNITS (id lists; a single word is a unit of length 1) -- ``required_phrases(ids)`` tells
    the two apart; under ``decoding_constraint`` a phrase that repeats a word and two items that could meet at a shared word are a ValueError naming them.  Without a
    phrase nothing changes.
    An item that contains ``|`` is a set of ALTERNATIVES ('dog|dogs|puppy', 'fire hydrant|hydrant'), any one of which satisfies it -- unless the vocabulary holds the
    whole item as one entry: then it is a plain word, ``|`` or not.  Each alternative resolves as an item does (a vocabulary entry that equals the whole alternative wins
    over splitting at spaces, 1 to 4 words, an unknown word is named); at most 4 of them, none given twice for an image.  If any image has such an item the whole
    evaluation goes through ``decode_many(require_any=...)`` and the result is (ids, words, texts): every entry of ``ids`` is a list of GROUPS (lists of alternatives, each
    an id list; a plain item is a group of one alternative) -- ``required_any(ids)`` tells --, ``texts`` holds every group's alternatives as text.  Under
    ``decoding_constraint`` an alternative that repeats a word and two alternatives of different items that could meet at a shared word are a ValueError naming them.
    Without a ``|`` item nothing changes."""
    spec = eval_kwargs.get("require_words")
    if not spec:
        return None
    if isinstance(spec, str):
        spec = [w for w in spec.split(",") if w]
    if isinstance(spec, dict):
        per_image = []
        for k in keys:
            ws = spec.get(k, spec.get(str(k), []))
            per_image.append([w for w in ws.split(",") if w] if isinstance(ws, str) else list(ws))
    else:
        per_image = [list(spec)] * len(keys)
    if not any(per_image):
        return None
    require_refusals(eval_kwargs, mode, sample_n)
    if not vocab:
        raise ValueError("require_words need a vocabulary ({str(id): word})")
    id_of = {}
    for k, w in vocab.items():
        id_of[w] = min(int(k), id_of.get(w, int(k)))
    ban = {int(i) for i in ban_ids or ()}
    def unit_of(w):
        parts = [w] if w in id_of else w.split()               # (a vocabulary entry that equals the whole item wins over splitting)
        for q in parts:
            if q not in id_of:
                raise ValueError(f"require_words: the vocabulary does not hold {q!r}")
            if id_of[q] in ban:
                raise ValueError(f"require_words: {q!r} is also banned (suppress_UNK / ban_words)")
        if not 1 <= len(parts) <= 4:
            raise ValueError(f"require_words: a phrase holds 1 to 4 words, got {w!r}")
        return [id_of[q] for q in parts]

    sets = lambda w: "|" in w and w not in id_of               # an item of alternatives (an item that is itself a vocabulary entry is a plain word)
    if any(sets(w) for ws in per_image for w in ws):
        return _required_any_of(eval_kwargs, per_image, unit_of, sets)
    ids, words = [], []
    for ws in per_image:
        ws = list(dict.fromkeys(ws))
        units = [unit_of(w) for w in ws]
        if len(ws) > 8:
            raise ValueError(f"require_words: at most 8 required words per image, got {len(ws)}")
        ids.append(units)
        words.append(ws)
    if not any(len(u) > 1 for units in ids for u in units):     # no phrase anywhere: single ids, as ever
        ids = [[u[0] for u in units] for units in ids]
    elif int(eval_kwargs.get("decoding_constraint", 0) or 0) == 1:      # what hip.require_unit_table refuses under no_repeat, said here in the items' words before anything is launched
        for units, ws in zip(ids, words):
            for a, u in enumerate(units):
                if any(x == y and x >= 7 for x, y in zip(u, u[1:])):
                    raise ValueError(f"require_words: {ws[a]!r} repeats a word (not under decoding_constraint)")
                for b in range(a):
                    v = units[b]
                    if (v[-1] == u[0] and u[0] >= 7) or (u[-1] == v[0] and v[0] >= 7):
                        raise ValueError(f"require_words: {ws[b]!r} and {ws[a]!r} could meet at a shared word and form an adjacent repeat (not under decoding_constraint)")
    return ids, words


def _required_any_of(eval_kwargs, per_image, unit_of, sets):
    """``required_of`` where some item is a set of alternatives: (ids, words, texts) -- per image the groups, the items, and every group's alternatives as text."""
    rep = int(eval_kwargs.get("decoding_constraint", 0) or 0) == 1
    ids, words, texts = [], [], []
    for ws in per_image:
        ws = list(dict.fromkeys(ws))
        groups, names, seen = [], [], []                         # seen: (item index, alternative's text, its ids) of the image so far
        for j, w in enumerate(ws):
            alts = [t for t in (a.strip() for a in w.split("|")) if t] if sets(w) else [w]
            if not alts:
                raise ValueError(f"require_words: {w!r} holds no alternative")
            if len(alts) > 4:
                raise ValueError(f"require_words: an item holds at most 4 alternatives, got {w!r}")
            group = []
            for t in alts:
                u = unit_of(t)
                for i, t2, v in seen:
                    if v == u:
                        raise ValueError(f"require_words: the alternative {t!r} is given twice" + (f" (in {ws[i]!r} and {w!r})" if i != j else f" in {w!r}"))
                    if rep and i != j and ((v[-1] == u[0] and u[0] >= 7) or (u[-1] == v[0] and v[0] >= 7)):
                        raise ValueError(f"require_words: {t2!r} and {t!r} could meet at a shared word and form an adjacent repeat (not under decoding_constraint)")
                if rep and any(x == y and x >= 7 for x, y in zip(u, u[1:])):
                    raise ValueError(f"require_words: {t!r} repeats a word (not under decoding_constraint)")
                seen.append((j, t, u))
                group.append(u)
            groups.append(group)
            names.append(alts)
        if len(ws) > 8:
            raise ValueError(f"require_words: at most 8 required words per image, got {len(ws)}")
        ids.append(groups)
        words.append(ws)
        texts.append(names)
    return ids, words, texts


def required_any(ids) -> bool:
    """Whether the ``ids`` of ``required_of`` are lists of groups of alternatives (some image has a ``|`` item) and go through ``require_any``."""
    return any(isinstance(a, list) for groups in ids for g in groups if isinstance(g, list) for a in g)


def required_key(ids) -> str:
    """The decode option that takes the ``ids`` of ``required_of``: 'require_any', 'require_phrases' or 'require_ids'."""
    return "require_any" if required_any(ids) else "require_phrases" if required_phrases(ids) else "require_ids"


def required_phrases(ids) -> bool:
    """Whether the ``ids`` of ``required_of`` are lists of units (some image has a phrase) and go through ``require_phrases``."""
    return any(isinstance(u, list) for units in ids for u in units)


def required_entry(words, pos_row, alt_row=None, texts=None):
    """The 'required' field of a prediction entry: [word or phrase, (start) position] per required item of the image, position None where it could not be placed.  With
    ``alt_row`` and ``texts`` (alternatives: the 'required_alt' row and the image's ``texts`` of ``required_of``): [item, start or None, the alternative placed (its
    text) or None]."""
    if alt_row is not None:
        return [[w, (int(p) if int(p) >= 0 else None), (t[int(a)] if int(p) >= 0 and 0 <= int(a) < len(t) else None)]
                for w, p, a, t in zip(words, pos_row[:len(words)].tolist(), alt_row[:len(words)].tolist(), texts)] if words else []
    return [[w, (int(p) if int(p) >= 0 else None)] for w, p in zip(words, pos_row[:len(words)].tolist())] if words else []


def required_rates(words, pos_rows, moved: int, emitted: int) -> dict:
    """required_rate = words (units, where phrases are required) placed / required, required_moved_rate = positions whose id the placement changed / positions emitted."""
    asked = sum(len(w) for w in words)
    placed = sum(sum(1 for p in row[:len(w)].tolist() if int(p) >= 0) for w, row in zip(words, pos_rows) if w)
    return {"required_rate": placed / max(1, asked), "required_moved_rate": moved / max(1, emitted)}


def eval_split(model, feats, store_or_gts, eval_kwargs, sample_n=None):
    """(val_loss, predictions, lang_stats) of ``feats``' images: see the module's head.  The model is put in eval() and restored."""
    kw = eval_kwargs
    sample_n = int(kw.get("sample_n", 1) if sample_n is None else sample_n)
    mode = kw.get("inference_mode", "NAIC")
    if mode not in ("NAIC", "SAIC"):
        raise NotImplementedError(f"inference mode {mode!r}: a UIC model decodes in 'NAIC' or 'SAIC' mode")
    batch_size, seq_per_img = int(kw.get("batch_size", 64)), int(kw.get("seq_per_img", 5))
    refine = {"refine_rounds": int(kw.get("refine_rounds", 0)), "refine_method": kw.get("refine_method", "feed_back")}
    if mode != "NAIC" and (refine["refine_rounds"] or refine["refine_method"] != "feed_back"):
        raise ValueError("refine_rounds / refine_method refine the non-autoregressive filling pass: inference_mode 'NAIC' only")
    n_method = sample_n_method_of(kw, mode, sample_n)
    nb_no_repeat = nbest_no_repeat_of(kw, sample_n)
    dv_lambda, dv_no_repeat = diverse_options_of(kw, sample_n)
    attn_topk = int(kw.get("attn_topk", 0))
    if attn_topk and mode != "NAIC":
        raise ValueError("attn_topk reads the non-autoregressive filling pass's cross-attention: inference_mode 'NAIC' only")
    if attn_topk:
        refine["attn_topk"] = attn_topk
    # suppress_UNK / decoding_constraint / ban_words / block_trigrams: the constrained pick (constraint_of); with language stats, constrained_rate = changed / emitted positions
    pick = constraint_of(kw, kw.get("vocab") or getattr(model, "vocab", None), mode, sample_n)
    refine.update(pick)
    # require_words: required words, phrases and alternatives (required_of) -- per-batch tables to decode_many (require_phrases when some image has a phrase, require_any when some item has '|': 'required' entries then hold the alternative placed as a third field); the predictions gain 'required' ([word, position or None] per word), the stats
    # required_rate and required_moved_rate (a dict of these two alone when no language scores were asked for).  Image keys: eval_kwargs['image_keys'], else 0 .. N - 1
    keys = kw.get("image_keys")
    required = required_of(kw, kw.get("vocab") or getattr(model, "vocab", None), list(keys) if keys is not None else list(range(len(feats))), mode, sample_n,
                           pick.get("ban_ids", ()))
    remove, surface_stats = int(kw.get("remove_bad_endings", 0)) == 1, int(kw.get("surface_stats", 0)) == 1
    if surface_stats and sample_n > 1 and kw.get("train_sentences") is None:
        raise ValueError("surface_stats with sample_n > 1 looks the sampled captions up among the training sentences: eval_kwargs['train_sentences'] "
                         "(a surface.TrainSentences) is missing")
    surface = caption_surface(model, kw) if remove or surface_stats else None
    rounds = []
    N = len(feats)
    ixs = kw.get("image_ixs")
    store = store_or_gts if hasattr(store_or_gts, "batch") and hasattr(store_or_gts, "gts") else None
    was_training = model.training
    model.eval()
    try:
        model.engine()                                           # the engine's packed weights follow the parameters (re-packed on the device if they moved)
        torch.cuda.synchronize()                                 # ... before any fork's stream reads them
        val_loss = 0.0
        if store is not None and kw.get("verbose_loss", 1):
            loss_sum, loss_evals = validation_loss(model, feats, store, batch_size, seq_per_img, ixs)
            val_loss = loss_sum / max(1, loss_evals)
        predictions, got = [], []
        vocab = kw.get("vocab")
        ragged = is_region_source(feats)
        host = feats if ragged else _torch_feats(feats)
        if required is not None:
            refine[required_key(required[0])] = [required[0][j:j + batch_size] for j in range(0, N, batch_size)]
        with torch.no_grad():
            if mode == "NAIC" and ragged:                       # staged ragged batch by batch, ahead of the launches that consume them
                for r in model.decode_many((feats.ragged(j, min(j + batch_size, N)) for j in range(0, N, batch_size)), batches_per_launch=int(kw.get("batches_per_launch", 16)),
                                           in_flight=kw.get("in_flight"), fused_vocab=bool(kw.get("fused_vocab", False)), **refine):
                    rounds.append(r.get("refine_round"))
                    got.append(r)
            elif mode == "NAIC":
                if host.dtype != torch.float32 and host.dtype != model.compute_dtype:
                    host = host.float()
                if model.compute_dtype == torch.bfloat16:     # (as a loader of half-precision feature files hands them over)
                    host = host.to(torch.bfloat16)
                if not host.is_cuda:
                    host = host.pin_memory()
                batches = [host[i:i + batch_size] for i in range(0, N, batch_size)]
                for r in model.decode_many(batches, batches_per_launch=int(kw.get("batches_per_launch", 16)), in_flight=kw.get("in_flight"),
                                           fused_vocab=bool(kw.get("fused_vocab", False)), **refine):
                    rounds.append(r.get("refine_round"))
                    got.append(r)
            else:
                for i in range(0, N, batch_size):
                    if ragged:
                        att, masks = device_batch(host, i, i + batch_size)
                    else:
                        att, masks = host[i:i + batch_size].cuda(), None
                    fc = torch.zeros(att.size(0), 0, device="cuda")
                    seq, lp, pn, pl, ps, _ = model(fc, att, masks, opt={"train_mode": "SAIC", "sample_method": "greedy", "sample_n": 1}, mode="sample")
                    # per-image entropy / perplexity as eval_utils.py:463-464, from the fused row reductions (bofi_vocab_stats)
                    ent, ppl = model.engine().entropy_perplexity({"seq": seq, "seq_logprob": lp})
                    got.append({"seq": seq.cpu(), "phrase_num": pn.cpu(), "phrase_length": pl.cpu(), "entropy": ent.cpu(), "perplexity": ppl.cpu()})
            # the batches' results are host tensors: with a surface option, ONE trim launch over the split's ids, before the entries and the scorers
            seqs, ents, ppls = [r["seq"] for r in got], [r["entropy"] for r in got], [r["perplexity"] for r in got]
            scored, bad = None, None
            if got and (remove or (surface_stats and int(kw.get("language_eval", 0)) == 1)):
                scored, _, bad = surface.trim(torch.cat(seqs), remove=remove)
                if remove:
                    seqs = list(torch.split(scored.cpu(), [s.size(0) for s in seqs]))
            i = 0
            for r, seq in zip(got, seqs):
                r = dict(r, seq=seq)
                predictions.extend(with_regions(entry_of(i, k, seq, r["phrase_num"], r["phrase_length"], r["entropy"], r["perplexity"], vocab), r, k) for k in range(seq.size(0)))
                if required is not None:
                    for k in range(seq.size(0)):
                        predictions[i + k]["required"] = (required_entry(required[1][i + k], r["required_pos"][k], *((r["required_alt"][k], required[2][i + k]) if "required_alt" in r else ()))
                                                          if "required_pos" in r else [])
                i += seq.size(0)
        if refine["refine_method"] == "mask_predict":
            kw["refine_round"] = torch.cat(rounds)
        lang_stats, ev = None, None
        if int(kw.get("language_eval", 0)) == 1:
            ev = kw.get("lang_eval")
            if ev is None:
                if store_or_gts is None:
                    raise ValueError("language_eval needs the images' references (a label source, or the references themselves)")
                gts = [store.gts(int(ixs[i]) if ixs is not None else i) for i in range(N)] if store is not None else list(store_or_gts)
                from .lang_eval import LanguageEval
                ev = kw["lang_eval"] = LanguageEval(gts, next(model.parameters()).device)
            lang_stats = ev.evaluate(scored if remove else torch.cat(seqs), torch.cat(ents), torch.cat(ppls))
        if sample_n > 1:                                         # eval_split_n + the div_stats / self_cider of language_eval (eval_utils.py:105-120)
            if n_method == "nbest":                              # the sample_n most probable captions of the filling pass in place of sample_n draws
                info = {}
                kw["preds_n"], sampled = sample_n_predictions(model, feats, sample_n, mode, batch_size, vocab, surface if remove else None, method="nbest",
                                                              ban_ids=pick.get("ban_ids"), refine_rounds=refine["refine_rounds"], info=info,
                                                              nbest_no_repeat=nb_no_repeat)
            elif n_method == "diverse":                          # a Hamming-diverse set of the filling pass's captions, group after group
                info = {}
                kw["preds_n"], sampled = sample_n_predictions(model, feats, sample_n, mode, batch_size, vocab, surface if remove else None, method="diverse",
                                                              ban_ids=pick.get("ban_ids"), refine_rounds=refine["refine_rounds"], info=info,
                                                              diversity_lambda=dv_lambda, diverse_no_repeat=dv_no_repeat)
            else:
                kw["preds_n"], sampled = sample_n_predictions(model, feats, sample_n, mode, batch_size, vocab, surface if remove else None)
            div, kw["diversity_per_image"] = diversity_stats(sampled, sample_n, kw)
            lang_stats = dict(lang_stats or {}, **div)
            if n_method == "nbest":
                lang_stats["nbest_short"] = kw["nbest_short"] = info["nbest_short"]
            if n_method == "diverse":
                lang_stats["diverse_short"] = kw["diverse_short"] = info["diverse_short"]
            if ev is not None and int(kw.get("eval_oracle", 0)) == 1:      # the oracle of language_eval (eval_utils.py:112-114): inside it, and only with a preds_n
                oracle = ev.evaluate_n(sampled, sample_n)
                kw["oracle_per_image"] = oracle.pop("per_image")
                lang_stats.update(oracle)
            if surface_stats:                                    # novel_sentences / vocab_size of language_eval (eval_utils.py:55-69), on the ids
                from .surface import sentence_stats
                canon, kept, _ = surface.trim(sampled, remove=False)      # (the canonical form of the -- already trimmed -- rows, and their lengths)
                lang_stats.update(sentence_stats(canon, kept, kw["train_sentences"], surface.V))
        if surface_stats and bad is not None and ev is not None:      # bad_count_rate (eval_utils.py:122): inside language_eval, of the scored captions
            lang_stats["bad_count_rate"] = surface.bad_count_rate(bad)
        if pick and lang_stats is not None:                      # after every other key
            lang_stats["constrained_rate"] = constrained_rate(got)
        if required is not None:
            rows = [row for r in got for row in (r["required_pos"] if "required_pos" in r else [torch.empty(0, dtype=torch.int32)] * r["seq"].size(0))]
            moved = sum(int(r["required_moved"].sum()) for r in got if "required_moved" in r)
            lang_stats = dict(lang_stats or {}, **required_rates(required[1], rows, moved, sum(int(r["phrase_length"].sum()) for r in got)))
    finally:
        model.train(was_training)
    return val_loss, predictions, lang_stats
