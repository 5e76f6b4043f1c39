#!/usr/bin/env python3
"""Entry point mirroring the reference's tools/eval.py (/root/reference/tools/eval.py:24-44,123) for the
path this repository implements: greedy NAIC bound+fill decoding of precomputed region features.

    python tools/eval.py --model model.pth [--infos_path infos.pkl] --inference_mode NAIC \\
        [--input_att_npy feats.npy | --input_att_dir DIR --input_json J [--split val] | --synthetic 64] [--batch_size 64] [--dtype bf16|f32] [--dump_json out.json]

`--model` is a state_dict written by the reference (311 entries) or by this repository.  Beam search is outside the scope of this build
(SURVEY.md §2).  Features come from a .npy of shape [N, R, 2048], are synthetic, or -- ``--input_att_dir D --input_json J [--split val|test|train]
[--num_images N] [--norm_att_feat 1]`` -- are the reference's per-image feature files (``<id>.npz`` / ``<id>.npy`` of 10..100 regions each, a ``.pth``
dictionary; boficap_amd.features): the images and their ids are the json's split, every batch is staged ragged by ``--feeder_workers`` reader threads and
padded on the device, ``image_id`` in the predictions is the json's id, and image i of the split uses image ``split_ix[i]`` of ``--input_label_npz``.
Box features: ``--use_box 1 --input_box_dir D [--input_box_ext .npy] [--norm_box_feat 1]`` reads ``<id>.npy`` boxes [r, 4] = (x1, y1, x2, y2) and the json's
``width`` / ``height``; the five geometry columns, the sort by box area and the zero-padding of F = 2053 to the engine's 2112 are the same device launch
(the model's ``att_feat_size`` must be 2053; no validation loss: ``mode='forward'`` is not built for that width).  ``--language_eval 1`` (with ``--input_label_npz``: the references) adds the language scores that need no Java -- BLEU-1..4,
ROUGE-L, CIDEr on the device (boficap_amd.lang_eval) -- as a printed line and, in ``--dump_json``, under a top-level key.
``--attn_topk K`` (NAIC) adds 'regions' to every prediction: per emitted word the K image regions its position attended to most, as [region, weight] pairs.
``--refine_rounds N [--refine_method feed_back|mask_predict]`` (NAIC) adds N filling passes: on all of the previous ids, or -- mask-predict -- on the least
confident positions only.
``--sample_n N`` (N > 1, with ``--cached_tokens``: the document frequencies) draws N captions per image after the greedy pass and adds their
diversity statistics -- Div-1, Div-2, mBLEU-1..4, self-CIDEr on the device (boficap_amd.diversity) -- the same way, with the sampled captions under
``preds_n``.  ``--eval_oracle 1`` (with ``--language_eval 1 --sample_n N``) scores every sampled caption against its image's references and adds
the best of an image's N and their mean per metric (``oracle_<M>``, ``avg_<M>``: boficap_amd.lang_eval.LanguageEval.evaluate_n) as one more line.
``--remove_bad_endings 1`` strips every caption's trailing function words on the device (the reference's REMOVE_BAD_ENDINGS; boficap_amd.surface) before it is
scored and dumped; ``--surface_stats 1`` adds ``bad_count_rate`` (with ``--language_eval 1``) and, with ``--sample_n N``, ``novel_sentences`` and ``vocab_size``
of the sampled captions against the training sentences: the captions in ``--input_label_npz`` of every image of ``--input_json`` whose split is neither val nor
test.  Both need the words' ids: ``--infos_path`` (a vocabulary), or ``--bad_endings W1,W2,...``, which overrides the trimmed word set for other vocabularies.
``--require_words W1,W2,...`` (every image) or ``--require_words_json FILE`` ({image id: [words]}) (NAIC) places the words in the captions where they cost the least
log-prob (boficap_amd.eval_utils.required_of; at most 8 per image): the predictions gain ``required`` ([word, position or null] per word) and a line reports
``required_rate`` (words placed / words required) and ``required_moved_rate``.  An item with a space is a phrase of up to 4 words (``"fire hydrant,dog"``): its
words go side by side on the cheapest span, ``required`` holds [phrase, start position or null], and the rates count units.  An item with ``|`` is a set of up to 4
alternatives, any one of which satisfies it (``"dog|dogs,fire hydrant|hydrant"``): the cheapest one is placed, ``required`` holds [item, start position or null, the
alternative placed or null], and the rates count items.
``--sample_n N --sample_n_method nbest`` (NAIC, N <= 8) takes the N most probable captions of the filling pass -- exact, from one decode -- in place of N random
draws: ``preds_n`` entries gain ``logp``, the statistics ``nbest_short``.
``--nbest_no_repeat 1`` (with ``--sample_n_method nbest``, N <= 6) makes that list the N most probable captions with no adjacent repeated word -- exact too (a
list-Viterbi over each row's N + 2 best ids); the greedy predictions stay the plain decode's.  An argument error without ``--sample_n_method nbest`` or with N > 6.
``--sample_n N --sample_n_method diverse`` (NAIC, N <= 8) takes a Hamming-diverse set of N captions -- the reference's diverse beam search ('dbs', one beam per group)
where it is exact: group g maximises its log-prob minus ``--diversity_lambda`` (0.5) times the earlier groups that put the same word at the same position; caption 0
is the greedy one.  ``--diverse_no_repeat 1`` (N <= 6) keeps adjacent repeated words out of every caption of the set.  ``preds_n`` entries gain ``logp``, the
statistics ``diverse_short``.
"""
import argparse
import json
import os
import pickle
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="", help="path to model.pth (state_dict); empty = seeded synthetic weights")
    ap.add_argument("--infos_path", default="", help="infos_*.pkl of the reference (opt namespace + vocab)")
    ap.add_argument("--inference_mode", default="NAIC", choices=["NAIC", "SAIC"])
    ap.add_argument("--input_att_npy", default="")
    ap.add_argument("--input_att_dir", default="", help="the reference's input_att_dir: a directory of <id>.npz (key 'feat', else 'z') or <id>.npy, or a .pth key -> array "
                    "dictionary (.h5 / .lmdb with h5py / lmdbdict); needs --input_json")
    ap.add_argument("--input_att_ext", default=".npz", choices=[".npz", ".npy"], help="file type of a feature directory")
    ap.add_argument("--input_json", default="", help="the preprocessing's json: images[*]['id'] and ['split']")
    ap.add_argument("--split", default="val", choices=["val", "test", "train"])
    ap.add_argument("--num_images", type=int, default=-1, help="the first N images of the split (-1: all)")
    ap.add_argument("--norm_att_feat", type=int, default=0, choices=[0, 1], help="1: every region divided by its L2 norm (dataloader.py:475-476), on the device")
    ap.add_argument("--use_box", type=int, default=0, choices=[0, 1], help="1 (with --input_att_dir and --input_box_dir): five box-geometry columns behind the 2048 region "
                    "features and every image's regions sorted by box area (dataloader.py:477-487), on the device; the model's att_feat_size is 2053")
    ap.add_argument("--input_box_dir", default="", help="the reference's input_box_dir: <id>.npy (or .npz) of [regions, 4] = x1, y1, x2, y2 in pixels; the json needs width and height")
    ap.add_argument("--input_box_ext", default=".npy", choices=[".npz", ".npy"], help="file type of the box directory")
    ap.add_argument("--norm_box_feat", type=int, default=0, choices=[0, 1], help="1: the five box columns divided by their L2 norm (dataloader.py:483-484), on the device")
    ap.add_argument("--in_memory", type=int, default=0, choices=[0, 1], help="1: every feature file is read once before the decode and served from memory")
    ap.add_argument("--feeder_workers", type=int, default=4, help="reader threads of the feature files (at most 16)")
    ap.add_argument("--synthetic", type=int, default=64)
    ap.add_argument("--batch_size", type=int, default=64)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--dump_json", default="")
    ap.add_argument("--input_label_npz", default="", help="label arrays (schema of scripts/prepro_labels_stanford.py:393-399, as .npz, or .h5 with h5py): "
                    "also report the validation loss of eval_split (eval_utils.py:440-453); image i of the features = image i of the file")
    ap.add_argument("--seq_per_img", type=int, default=5)
    ap.add_argument("--pipeline", type=int, default=1, help="1 (default, NAIC): the batches go through TransformerModel.decode_many -- 4 launches in flight, 16 batches per "
                    "launch, features copied from pinned host memory ahead of the launches; 0: one synchronised mode='sample' call per batch as the reference's eval loop "
                    "(eval_utils.py:456-460)")
    ap.add_argument("--batches_per_launch", type=int, default=16)
    ap.add_argument("--in_flight", type=int, default=3, help="launch streams (3 launch streams + the copy stream = the runtime's default of 4 hardware queues)")
    ap.add_argument("--fused_vocab", action="store_true", help="pipelined NAIC only: ids-only launches -- generator and vocabulary epilogue as one launch that writes no "
                    "logits, forks without the vocabulary-wide buffers (TransformerModel.decode_many(fused_vocab=True))")
    ap.add_argument("--language_eval", type=int, default=0, choices=[0, 1], help="1: BLEU-1..4, ROUGE-L and CIDEr of the captions against the references of "
                    "--input_label_npz; --dump_json then holds {'predictions': [...], 'lang_stats': {...}} instead of the list")
    ap.add_argument("--sample_n", type=int, default=1, help="N > 1: after the greedy pass draw N captions per image (sample_method 'sample') and report Div-1, Div-2, "
                    "mBLEU-1..4 and self-CIDEr over them; --dump_json then holds {'predictions', 'preds_n', 'lang_stats'}")
    ap.add_argument("--sample_n_method", default="sample", choices=["sample", "nbest", "diverse"], help="what the N captions of --sample_n are: 'sample' = N random draws; "
                    "'diverse' (NAIC only, N <= 8) = a Hamming-diverse set, decoded group after group from ONE decode: each caption maximises its log-prob minus "
                    "--diversity_lambda times the earlier captions with the same word at the same position (the reference's 'dbs' with one beam per group, exact here); "
                    "entries gain 'logp', the statistics diverse_short; refusals as 'nbest'; "
                    "'nbest' (NAIC only, N <= 8) = the N most probable captions of the filling pass, most probable first, exact and from ONE decode -- every entry of "
                    "preds_n gains 'logp', the statistics nbest_short (images with fewer than N distinct captions); --suppress_UNK / --ban_words apply to the list, "
                    "not with --decoding_constraint / --block_trigrams / --refine_method mask_predict / --require_words")
    ap.add_argument("--nbest_no_repeat", type=int, default=0, choices=[0, 1], help="1 (with --sample_n_method nbest, --sample_n <= 6): the list is of the captions "
                    "with no adjacent repeated word (ids >= 7), the N most probable of them, exactly; the greedy predictions stay the plain decode's")
    ap.add_argument("--diversity_lambda", type=float, default=0.5, help="with --sample_n_method diverse: the penalty per earlier caption of the set that has the same word "
                    "at the same position (the reference's option and default); finite and >= 0")
    ap.add_argument("--diverse_no_repeat", type=int, default=0, choices=[0, 1], help="1 (with --sample_n_method diverse, --sample_n <= 6): no caption of the set has an "
                    "adjacent repeated word (ids >= 7); the greedy predictions stay the plain decode's")
    ap.add_argument("--cached_tokens", default="coco-train-idxs", help="document-frequency pickle of the self-CIDEr score (scripts/prepro_ngrams.py): a path, or a "
                    "name resolved as data/<name>.p")
    ap.add_argument("--eval_oracle", type=int, default=0, choices=[0, 1], help="1 (with --language_eval 1 --sample_n N): oracle_<M> and avg_<M>, the best and the "
                    "mean of an image's N sampled captions, for BLEU-1..4, ROUGE-L and CIDEr against the references")
    ap.add_argument("--refine_rounds", type=int, default=0, help="NAIC only: N extra filling passes (0..15) after the first")
    ap.add_argument("--refine_method", default="feed_back", choices=["feed_back", "mask_predict"], help="what the extra passes are: 'feed_back' decodes again on all of the "
                    "previous ids; 'mask_predict' (needs --refine_rounds >= 1) re-predicts only each caption's least confident positions, fewer every pass, and keeps the rest")
    ap.add_argument("--attn_topk", type=int, default=0, help="NAIC only: K in 1..8 -- every prediction gains 'regions', per emitted word the [region, weight] pairs of the K "
                    "image regions its position attended to most (mean over heads of the last decoder layer's cross-attention), heaviest first")
    ap.add_argument("--remove_bad_endings", type=int, default=0, choices=[0, 1], help="1: every caption (greedy and sampled) loses its trailing run of bad-ending "
                    "words before it is scored and dumped; a caption of such words alone is left as it is")
    ap.add_argument("--surface_stats", type=int, default=0, choices=[0, 1], help="1: bad_count_rate (with --language_eval 1) and, with --sample_n N, novel_sentences "
                    "and vocab_size of the sampled captions (these need --input_label_npz and --input_json: the training sentences)")
    ap.add_argument("--bad_endings", default="", help="W1,W2,...: the words --remove_bad_endings strips, instead of the reference's list")
    ap.add_argument("--suppress_UNK", type=int, default=0, choices=[0, 1], help="NAIC only: 1 = no caption holds UNK -- every position takes its best other word (the "
                    "reference's option, which does nothing on its non-autoregressive path; so the default here is 0, not its 1: the defaults keep the captions)")
    ap.add_argument("--decoding_constraint", type=int, default=0, choices=[0, 1], help="NAIC only: 1 = no word stands twice in a row -- a position that would repeat its "
                    "left neighbour takes its second-best word (the reference's option, applied there on the autoregressive paths only)")
    ap.add_argument("--block_trigrams", type=int, default=0, choices=[0, 1], help="NAIC only: 1 = no word trigram stands twice in a caption -- a position whose two left "
                    "neighbours repeat an earlier pair of words does not take the word that followed that pair (the reference's option, applied there on the autoregressive "
                    "paths only and as a penalty; here a hard block)")
    ap.add_argument("--ban_words", default="", help="NAIC only: W1,W2,... never appear in a caption (resolved to ids as --bad_endings resolves its words)")
    ap.add_argument("--require_words", default="", help="NAIC only: W1,W2,... appear in every caption -- each placed on the position where it costs the least log-prob; "
                    "an item with a space is a phrase of up to 4 words ('fire hydrant,dog'), placed side by side on the cheapest span; an item with '|' is a set of up to 4 alternatives, any one of which "
                    "satisfies it ('dog|dogs,fire hydrant|hydrant'): the cheapest is placed "
                    "(eval_kwargs['require_words']; the predictions gain 'required', the statistics required_rate and required_moved_rate)")
    ap.add_argument("--require_words_json", default="", help="NAIC only: a JSON file {image id: [W1, W2, ...]} of required words, phrases and alternatives ('dog|dogs') per image (the ids of --input_json, else "
                    "the images' indices); not together with --require_words")
    args = ap.parse_args()
    if args.require_words and args.require_words_json:
        ap.error("--require_words and --require_words_json are two sources of the same words: give one")
    if args.require_words or args.require_words_json:
        try:
            from boficap_amd import eval_utils as _eu
            _eu.require_refusals(vars(args), args.inference_mode, args.sample_n)
        except ValueError as e:
            ap.error("--require_words / --require_words_json: " + str(e))
    try:
        from boficap_amd import eval_utils as _eu
        _eu.sample_n_method_of(vars(args), args.inference_mode, args.sample_n)
    except ValueError as e:
        ap.error("--sample_n_method: " + str(e))
    try:
        nbest_no_repeat = _eu.nbest_no_repeat_of(vars(args), args.sample_n)
    except ValueError as e:
        ap.error("--nbest_no_repeat: " + str(e))
    try:
        diversity_lambda, diverse_no_repeat = _eu.diverse_options_of(vars(args), args.sample_n)
    except ValueError as e:
        ap.error("--diversity_lambda / --diverse_no_repeat: " + str(e))
    try:                                                         # (before anything is loaded; the words are resolved once the vocabulary is)
        from boficap_amd import eval_utils as _eu
        _eu.constraint_of(vars(args), {"0": "UNK"}, args.inference_mode, args.sample_n)
    except ValueError as e:
        ap.error("--suppress_UNK / --decoding_constraint / --ban_words / --block_trigrams: " + str(e))
    if (args.remove_bad_endings or args.surface_stats) and not (args.infos_path or args.bad_endings):
        ap.error("--remove_bad_endings / --surface_stats need the ids of the bad-ending words: --infos_path (a vocabulary) or --bad_endings W1,W2,...")
    if args.surface_stats and args.sample_n > 1 and not (args.input_label_npz and args.input_json):
        ap.error("--surface_stats 1 with --sample_n N looks the sampled captions up among the training sentences: it needs --input_label_npz and --input_json")
    if args.attn_topk and args.inference_mode != "NAIC":
        ap.error("--attn_topk reads the non-autoregressive filling pass's cross-attention: it needs --inference_mode NAIC")
    if not 0 <= args.attn_topk <= 8:
        ap.error("--attn_topk must be in 0..8")
    if (args.refine_rounds or args.refine_method != "feed_back") and args.inference_mode != "NAIC":
        ap.error("--refine_rounds / --refine_method refine the non-autoregressive filling pass: they need --inference_mode NAIC")
    if not 0 <= args.refine_rounds <= 15 or (args.refine_method == "mask_predict" and args.refine_rounds < 1):
        ap.error("--refine_rounds must be in 0..15, and --refine_method mask_predict needs at least 1")
    refine = {"refine_rounds": args.refine_rounds, "refine_method": args.refine_method}
    if args.attn_topk:                                           # (rides with the refinement options: decode_many and mode='sample' take it the same way)
        refine["attn_topk"] = args.attn_topk
    if args.language_eval and not args.input_label_npz:
        ap.error("--language_eval 1 needs the references: --input_label_npz")
    if args.use_box and not (args.input_box_dir and args.input_att_dir):
        ap.error("--use_box 1 makes F = 2053 from the boxes of the images' regions: it needs --input_box_dir (and --input_att_dir, --input_json with width and height)")
    if (args.input_box_dir or args.norm_box_feat) and not args.use_box:
        ap.error("--input_box_dir / --norm_box_feat are read with --use_box 1 only")
    if args.input_att_dir and not args.input_json:
        ap.error("--input_att_dir needs the images' ids and splits: --input_json")
    if args.input_att_dir and args.input_att_npy:
        ap.error("--input_att_dir and --input_att_npy are two sources of the same features: give one")
    if args.eval_oracle and not (args.language_eval and args.sample_n > 1):
        ap.error("--eval_oracle 1 scores the sampled captions against the references: it needs --language_eval 1 and --sample_n N (N > 1)")

    import captioning.models as models
    from boficap_amd import eval_utils, weights as W
    from boficap_amd.config import FULL

    vocab = None
    if args.infos_path:
        with open(args.infos_path, "rb") as f:
            infos = pickle.load(f, encoding="latin1")
        opt, vocab = infos["opt"], infos["vocab"]
        opt.vocab = vocab
    else:
        opt = FULL.to_opt()
    opt.bofi_compute_dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    opt.bofi_max_batch = args.batch_size
    image_ixs, image_ids, att_store = None, None, None
    if args.input_att_dir:
        from boficap_amd.features import ImageIndex, RegionFeeder, RegionSource, RegionStore
        index = ImageIndex(args.input_json)
        image_ixs = index.split_ix[args.split][:args.num_images if args.num_images >= 0 else None]
        if not image_ixs:
            raise SystemExit(f"{args.input_json} assigns no image to split {args.split!r}")
        image_ids = [index.ids[i] for i in image_ixs]
        att_store = RegionStore(args.input_att_dir, args.input_att_ext, in_memory=bool(args.in_memory))
        box_store, sizes = None, None
        if args.use_box:
            box_store = RegionStore(args.input_box_dir, args.input_box_ext, in_memory=bool(args.in_memory))
            sizes = index.sizes(image_ixs)
        box_kw = dict(box_store=box_store, norm_box_feat=bool(args.norm_box_feat))
        feats = RegionSource(att_store, image_ids, bool(args.norm_att_feat), sizes=sizes, **box_kw)
        if args.in_memory:
            for k in feats.keys:
                att_store.get(k)
                if box_store is not None:
                    box_store.get(k)
        # the width the files make against the width the model was built for (the reference's files: 2048 + 5 x use_box), before anything is loaded
        file_F = int(att_store.get(feats.keys[0]).shape[1])
        if int(opt.att_feat_size) != file_F + 5 * args.use_box:
            ap.error(f"the model's att_feat_size is {int(opt.att_feat_size)}, but the region files hold {file_F} columns and --use_box {args.use_box} makes "
                     f"features of {file_F + 5 * args.use_box}: a model trained with use_box {1 - args.use_box}?")
    model = models.setup(opt)
    if args.model:
        model.load_state_dict(torch.load(args.model, map_location="cpu"), strict=True)
    else:
        model.load_state_dict({k: torch.from_numpy(v) for k, v in W.make_state_dict(model.cfg, 0).items()}, strict=True)
    model.cuda().eval()

    if args.input_att_npy:
        feats = np.load(args.input_att_npy)
    elif not args.input_att_dir:                                 # (2 048 distinct synthetic images, repeated: the generator is a CPU loop)
        uniq = W.synthetic_att_feats(min(args.synthetic, 2048), 36, model.cfg.att_feat_size, seed=1235)
        feats = uniq if args.synthetic <= 2048 else np.concatenate([uniq] * (-(-args.synthetic // 2048)))[:args.synthetic]
    store = None
    if args.input_label_npz:
        from boficap_amd.data import LabelStore
        c = model.cfg
        src = args.input_label_npz if args.input_label_npz.endswith((".h5", ".hdf5")) else dict(np.load(args.input_label_npz))
        store = LabelStore(src, pad_idx=c.pad_idx, bos_idx=c.bos_idx, eos_idx=c.eos_idx, len_idx=c.len_idx)
    pick = eval_utils.constraint_of(vars(args), vocab or opt.vocab, args.inference_mode, args.sample_n)
    pick_opt = {"ban_ids": pick["ban_ids"], "decoding_constraint": int(pick["no_repeat"]), "block_trigrams": int(pick.get("block_trigrams", False))} if pick else {}      # (the same, in mode='sample''s names)
    # --require_words / --require_words_json: per-batch id tables for decode_many (opt['require_ids'] per call on the synchronised path)
    required, req_kw, req_pos, req_moved, req_alt = None, [], [], 0, []
    if args.require_words or args.require_words_json:
        if args.require_words_json:
            with open(args.require_words_json) as f:
                req_spec = json.load(f)
        else:
            req_spec = args.require_words
        try:
            required = eval_utils.required_of({**vars(args), "require_words": req_spec}, vocab or opt.vocab, image_ids if image_ids is not None else list(range(len(feats))),
                                              args.inference_mode, args.sample_n, pick.get("ban_ids", ()))
        except ValueError as e:
            ap.error(str(e))
        if required is not None:
            req_kw = [required[0][i:i + args.batch_size] for i in range(0, len(feats), args.batch_size)]
            req_key = eval_utils.required_key(required[0])      # (an item with a space is a phrase: units of ids; an item with '|' a group of alternatives)

    def req(n=None):
        return {req_key: req_kw[:n]} if required is not None else {}
    changed, emitted = 0, 0
    results, seconds, rows, stats = [], 0.0, [], ([], [])
    store_loss = store is not None and not args.use_box          # (mode='forward' is not built for F = 2053: box features are decode-only)
    surface, bad_flags = None, []
    if args.remove_bad_endings or args.surface_stats:
        from boficap_amd.surface import CaptionSurface, TrainSentences, sentence_stats
        words = vocab or opt.vocab
        surface = CaptionSurface.from_vocab(words, max(int(model.cfg.tgt_vocab), 1 + max(int(k) for k in words)), "cuda",
                                            trim_words=[w for w in args.bad_endings.split(",") if w] if args.bad_endings else None)

    def surfaced(batches):
        """The decoded batches with their ids trimmed (--remove_bad_endings): one launch over all of them; their bad-ending flags are kept."""
        if surface is None or not batches:
            return batches
        out, _, bad = surface.trim(torch.cat([r["seq"] for r in batches]), remove=bool(args.remove_bad_endings))
        bad_flags.append(bad)
        if not args.remove_bad_endings:
            return batches
        return [dict(r, seq=seq) for r, seq in zip(batches, torch.split(out.cpu(), [r["seq"].size(0) for r in batches]))]

    def entry_of(i, k, seq, pn, pl, ent, ppl):
        if args.language_eval and k == 0:                        # (the batch's raw rows, for the language scores)
            rows.append(seq.cpu()); stats[0].append(ent.cpu()); stats[1].append(ppl.cpu())
        return eval_utils.entry_of(i, k, seq, pn, pl, ent, ppl, vocab)

    with torch.no_grad():
        if store_loss:                   # the loss of eval_split (verbose_loss), eval_utils.py:440-453: a pass of its own
            loss_sum, loss_evals = eval_utils.validation_loss(model, feats, store, args.batch_size, args.seq_per_img, image_ixs)
        if args.pipeline and args.inference_mode == "NAIC" and att_store is not None:
            # the feature files are read and staged ragged by the feeder's threads INSIDE the clock, ahead of the launches; padding and cast happen on the device
            key_batches = [feats.keys[i:i + args.batch_size] for i in range(0, len(feats), args.batch_size)]

            def feeder(kb):
                return RegionFeeder(att_store, kb, workers=args.feeder_workers, norm_att_feat=bool(args.norm_att_feat),
                                    sizes=None if sizes is None else {k: wh for k, wh in zip(feats.keys, sizes)}, **box_kw)
            for _ in model.decode_many(feeder(key_batches[:2 * args.in_flight * args.batches_per_launch]), batches_per_launch=args.batches_per_launch, in_flight=args.in_flight,
                                       fused_vocab=args.fused_vocab, **refine, **pick, **req(2 * args.in_flight * args.batches_per_launch)):
                pass                                             # graph captures and stream choice, outside the clock
            torch.cuda.synchronize()
            import time
            t0 = time.time()
            got = list(model.decode_many(feeder(key_batches), batches_per_launch=args.batches_per_launch, in_flight=args.in_flight, fused_vocab=args.fused_vocab, **refine, **pick, **req()))
            seconds = time.time() - t0
            i = 0
            for r in surfaced(got):
                n = r["seq"].size(0)
                results.extend(eval_utils.with_regions(entry_of(i, k, r["seq"], r["phrase_num"], r["phrase_length"], r["entropy"], r["perplexity"]), r, k) for k in range(n))
                i += n
            how = (f"pipelined: {args.in_flight} launches in flight, {args.batches_per_launch} batches of {args.batch_size} per launch, feature files read by {args.feeder_workers} "
                   f"threads and staged ragged, file reads and host results included" + (", fused vocabulary epilogue" if args.fused_vocab else ""))
        elif args.pipeline and args.inference_mode == "NAIC":
            # the features as a loader of half-precision feature files hands them over: compute dtype, pinned host memory (staged once, outside the clock --
            # float32 features would cross PCIe at twice the bytes: ~190 k images/s at 55 GB/s)
            host = torch.from_numpy(np.ascontiguousarray(feats))
            if args.dtype == "bf16":
                host = host.to(torch.bfloat16)
            host = host.pin_memory()
            batches = [host[i:i + args.batch_size] for i in range(0, host.size(0), args.batch_size)]
            for _ in model.decode_many(batches[:2 * args.in_flight * args.batches_per_launch], batches_per_launch=args.batches_per_launch, in_flight=args.in_flight, fused_vocab=args.fused_vocab, **refine, **pick,
                                       **req(2 * args.in_flight * args.batches_per_launch)):
                pass                                             # graph captures and stream choice, outside the clock
            torch.cuda.synchronize()
            import time
            t0, got = time.time(), []
            for r in model.decode_many(batches, batches_per_launch=args.batches_per_launch, in_flight=args.in_flight, fused_vocab=args.fused_vocab, **refine, **pick, **req()):
                got.append(r)                                    # host tensors of one batch: ids, slot layout, entropy, perplexity
            seconds = time.time() - t0
            i = 0
            for r in surfaced(got):                              # (the JSON entries are built outside the clock: ~20 us of Python per image)
                n = r["seq"].size(0)
                results.extend(eval_utils.with_regions(entry_of(i, k, r["seq"], r["phrase_num"], r["phrase_length"], r["entropy"], r["perplexity"]), r, k) for k in range(n))
                i += n
            how = f"pipelined: {args.in_flight} launches in flight, {args.batches_per_launch} batches of {args.batch_size} per launch, features from pinned host memory, host results included" + (", fused vocabulary epilogue" if args.fused_vocab else "")
        else:
            for i in range(0, len(feats), args.batch_size):
                if att_store is not None:
                    att, masks = eval_utils.device_batch(feats, i, i + args.batch_size)
                else:
                    att, masks = torch.from_numpy(np.ascontiguousarray(feats[i:i + args.batch_size])).cuda(), None
                fc = torch.zeros(att.size(0), 0, device="cuda")
                seq, lp, pn, pl, ps, t = model(fc, att, masks, opt=dict({"train_mode": args.inference_mode, "sample_method": "greedy", "sample_n": 1},
                                                                                   **(dict(refine, **pick_opt) if args.inference_mode == "NAIC" else {}),
                                                                                   **({req_key: req_kw[i // args.batch_size]} if required is not None else {})), mode="sample")
                seconds += t
                if required is not None:
                    b = att.size(0)
                    last = model.last_required
                    req_pos.extend(last["pos"].cpu() if last is not None else [torch.empty(0, dtype=torch.int32)] * b)
                    req_moved += int(last["moved"].sum()) if last is not None else 0
                    if req_key == "require_any":
                        req_alt.extend(last["alt"].cpu() if last is not None else [torch.empty(0, dtype=torch.int32)] * b)
                    emitted += 0 if pick else int(pl.sum())
                if pick:
                    changed, emitted = changed + int(model.last_constrained.sum()), emitted + int(pl.sum())
                # per-image entropy / perplexity as eval_utils.py:463-464, from the fused row reductions (bofi_vocab_stats); under mask-predict from the statistics of
                # the pass that emitted each token (the log-prob tensor is the last pass's)
                if args.refine_method == "mask_predict":
                    ent, ppl = model.engine().entropy_perplexity({"seq": seq, "_row_stats_fused": True, "row_plogp": model.last_refine_row_stats[0], "row_chosen": model.last_refine_row_stats[1]})
                else:
                    ent, ppl = model.engine().entropy_perplexity({"seq": seq, "seq_logprob": lp})
                r = surfaced([{"seq": seq.cpu(), **({k2: model.last_attn[k2].cpu() for k2 in ("attn_top", "attn_top_w")} if args.attn_topk else {})}])[0]
                results.extend(eval_utils.with_regions(entry_of(i, k, r["seq"], pn, pl, ent, ppl), r, k) for k in range(att.size(0)))
            how = "one synchronised mode='sample' call per batch (the reference's eval loop), decode time only"
    if pick and args.pipeline:
        changed, emitted = sum(int(r["constrained"].sum()) for r in got), sum(int(r["phrase_length"].sum()) for r in got)
    if required is not None and args.pipeline and args.inference_mode == "NAIC":
        emitted = sum(int(r["phrase_length"].sum()) for r in got)
        req_pos = [row for r in got for row in (r["required_pos"] if "required_pos" in r else [torch.empty(0, dtype=torch.int32)] * r["seq"].size(0))]
        req_moved = sum(int(r["required_moved"].sum()) for r in got if "required_moved" in r)
        if req_key == "require_any":
            req_alt = [row for r in got for row in (r["required_alt"] if "required_alt" in r else [torch.empty(0, dtype=torch.int32)] * r["seq"].size(0))]
    if required is not None and req_key == "require_any":
        for e, ws, row, alt, texts in zip(results, required[1], req_pos, req_alt, required[2]):
            e["required"] = eval_utils.required_entry(ws, row, alt, texts)
    elif required is not None:
        for e, ws, row in zip(results, required[1], req_pos):
            e["required"] = eval_utils.required_entry(ws, row)
    if image_ids is not None:                                    # the json's ids, in the split's order
        for e, iid in zip(results, image_ids):
            e["image_id"] = iid
    print(f"decoded {len(results)} images in {seconds:.4f} s ({len(results) / max(seconds, 1e-9):.1f} images/s; {how})")
    if store_loss:
        print(f"validation loss {loss_sum / max(1, loss_evals):.4f} over {loss_evals} batches (LanguageModelCriterion_UIC)")
    lang_stats = None
    if args.language_eval:
        from boficap_amd.lang_eval import LanguageEval
        lang_ev = LanguageEval([store.gts(image_ixs[i] if image_ixs is not None else i) for i in range(len(results))], "cuda")
        lang_stats = lang_ev.evaluate(torch.cat(rows), torch.cat(stats[0]), torch.cat(stats[1]))
        print("language scores " + " ".join(f"{k} {v:.6f}" for k, v in lang_stats.items()))
    preds_n = None
    if args.sample_n > 1:
        nb_info = {}
        preds_n, sampled = eval_utils.sample_n_predictions(model, feats, args.sample_n, args.inference_mode, args.batch_size, vocab,
                                                           surface if args.remove_bad_endings else None, method=args.sample_n_method,
                                                           ban_ids=pick.get("ban_ids") if pick else None, refine_rounds=args.refine_rounds, info=nb_info,
                                                           nbest_no_repeat=nbest_no_repeat, diversity_lambda=diversity_lambda, diverse_no_repeat=diverse_no_repeat)
        for e in preds_n:                                        # (an empty row past an image's count has logp -inf: null in the dump)
            if "logp" in e and not np.isfinite(e["logp"]):
                e["logp"] = None
        if image_ids is not None:
            for e in preds_n:
                e["image_id"] = image_ids[e["image_id"]]
        div, _ = eval_utils.diversity_stats(sampled, args.sample_n, {"cached_tokens": args.cached_tokens})
        lang_stats = dict(lang_stats or {}, **div)
        print("diversity scores " + " ".join(f"{k} {v:.6f}" for k, v in div.items()))
        if "nbest_short" in nb_info:
            lang_stats["nbest_short"] = nb_info["nbest_short"]
            print(f"n-best lists: {nb_info['nbest_short']} of {len(results)} images have fewer than {args.sample_n} distinct captions (nbest_short)")
        if "diverse_short" in nb_info:
            lang_stats["diverse_short"] = nb_info["diverse_short"]
            print(f"diverse sets (lambda {diversity_lambda:g}): {nb_info['diverse_short']} of {len(results)} images have fewer than {args.sample_n} captions (diverse_short)")
        if args.eval_oracle:
            oracle = lang_ev.evaluate_n(sampled, args.sample_n)
            oracle.pop("per_image")
            lang_stats.update(oracle)
            print("oracle scores " + " ".join(f"{k} {v:.6f}" for k, v in oracle.items()))
    if args.surface_stats:
        surf = {}
        if args.sample_n > 1:                                    # the training sentences: every image of the json that is neither val nor test
            from boficap_amd.features import ImageIndex
            train_ixs = [ix for ix, img in enumerate(ImageIndex(args.input_json).images) if img.get("split") not in ("val", "test")]
            canon, kept, _ = surface.trim(sampled, remove=False)
            surf.update(sentence_stats(canon, kept, TrainSentences.from_store(store, train_ixs, "cuda"), surface.V))
        if args.language_eval:
            surf["bad_count_rate"] = surface.bad_count_rate(torch.cat(bad_flags))
        if surf:
            lang_stats = dict(lang_stats or {}, **surf)
            print("surface statistics " + " ".join(f"{k} {v:.6f}" for k, v in surf.items()))
    if pick:                                                     # positions the constrained pick changed over positions emitted; with language scores, their last key
        rate = changed / max(1, emitted)
        print(f"constrained pick: {changed} of {emitted} emitted positions changed (constrained_rate {rate:.6f})")
        if lang_stats is not None:
            lang_stats["constrained_rate"] = rate
    if required is not None:                                     # words placed over words required; positions the placement changed over positions emitted
        rates = eval_utils.required_rates(required[1], req_pos, req_moved, emitted)
        print(f"required words: required_rate {rates['required_rate']:.6f} required_moved_rate {rates['required_moved_rate']:.6f}")
        if lang_stats is not None:
            lang_stats.update(rates)
    if args.dump_json:
        with open(args.dump_json, "w") as f:
            if preds_n is not None:
                json.dump({"predictions": results, "preds_n": preds_n, "lang_stats": lang_stats}, f)
            else:
                json.dump({"predictions": results, "lang_stats": lang_stats} if args.language_eval else results, f)


if __name__ == "__main__":
    main()
