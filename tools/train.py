#!/usr/bin/env python3
"""Entry point mirroring the reference's tools/train.py for the XE phase of a UIC model
(/root/reference/tools/train.py:97-101 model + DataParallel, :150-170 schedules, :198-229 the step, :304-360 checkpoints).

    python tools/train.py [--cfg configs/uic_sd.yml] [--id run] [--checkpoint_path DIR] [--max_iters 100]
                          [--batch_size 10] [--seq_per_img 5] [--dtype bf16|f32] [--glancing_token 1] [--tiny]
    python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 tools/train.py ...     # data parallel

One process per GPU (RANK / LOCAL_RANK / WORLD_SIZE from the environment) instead of ``nn.DataParallel``: every rank
steps on its own shard of images and the gradients meet in one RCCL all-reduce over the flat gradient bucket
(boficap_amd/trainer.py).  Batches are synthetic captions in the loader's layout (boficap_amd/collate.py), or -- with
``--input_label_h5`` (the label file, or an .npz of the same arrays) -- real captions from the preprocessing's label file (boficap_amd/data.py), on synthetic
region features unless ``--input_att_dir D --input_json J [--norm_att_feat 1] [--train_only 0|1] [--feeder_workers 4]`` names the reference's per-image feature
files (boficap_amd/features.py; XE phase only: ``--self_critical_after`` is refused with them): the training images are then drawn from the json's train split, their features are read by a feeder's threads a few steps
ahead, staged ragged and padded on the device (``att_masks`` from the region counts, None when a batch's counts are equal), and the validation set is the
first ``--val_images_use`` images of the val split.  ``--cfg`` reads the reference's yml files including their ``_BASE_``
inheritance (captioning/utils/config.py:35-95).  ``--self_critical_after N`` switches to the self-critical step (loss_wrapper.py:181-230,
``structure_loss_weight: 1``) from iteration N on, scored by ``boficap_amd.loss_wrapper``'s installed scorer or, without one, by CIDEr-D
on the device (boficap_amd.cider) with the document frequencies of ``--cached_tokens`` / the cfg's ``cached_tokens`` (data/<name>.p of
scripts/prepro_ngrams.py, as the reference resolves it), plus BLEU-4 (boficap_amd.rewards) with the cfg's ``bleu_reward_weight`` > 0 (no
df file needed when ``cider_reward_weight`` is 0); with no such file for a CIDEr-D term, by token overlap with the ground-truth captions.
Checkpoints are the reference's files (captioning/utils/misc.py:87-102; with ``--val_images_use N`` every ``save_checkpoint_every`` iterations follow a validation pass as the
reference's loop runs it, :296-363 -- loss, SAIC and NAIC captions, with ``--language_eval 1`` BLEU / ROUGE-L / CIDEr on the device -- into
``histories['val_result_history']`` and ``infos['best_val_score']``, and the best one is kept as ``model-best.pth``): ``model.pth`` (311-entry state_dict), ``optimizer.pth``
(NoamOpt / torch Adam layout), ``infos_<id>.pkl``, ``histories_<id>.pkl``; ``--start_from`` resumes from either code base's directory.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="", help="yml with the reference's option names (configs/uic_sd.yml)")
    ap.add_argument("--id", default="bofi")
    ap.add_argument("--checkpoint_path", default="")
    ap.add_argument("--start_from", default="", help="directory holding model.pth / optimizer.pth to resume from")
    ap.add_argument("--max_iters", type=int, default=50)
    ap.add_argument("--batch_size", type=int, default=None, help="images per rank and step (uic_sd.yml: 10)")
    ap.add_argument("--seq_per_img", type=int, default=None)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"], help="GEMM operand dtype (fp32 accumulation and master weights either way)")
    ap.add_argument("--glancing_token", type=int, default=0, help="1: GLAT with the reference's unmasked-rate schedule start value")
    ap.add_argument("--unmasked_rate_start", type=float, default=0.5)
    ap.add_argument("--losses_log_every", type=int, default=10)
    ap.add_argument("--save_checkpoint_every", type=int, default=0)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--tiny", action="store_true", help="the small test configuration instead of the 512-d model")
    ap.add_argument("--no_graph", action="store_true", help="run the step eagerly instead of replaying one hipGraph per batch signature")
    ap.add_argument("--input_label_h5", default="", help="label file of scripts/prepro_labels_stanford.py (captions and phrase cuts; .h5 / .hdf5 needs h5py), or an .npz of "
                    "the same arrays")
    ap.add_argument("--input_att_dir", default="", help="the reference's input_att_dir: a directory of <id>.npz (key 'feat', else 'z') or <id>.npy, or a .pth key -> array "
                    "dictionary (.h5 / .lmdb with h5py / lmdbdict); needs --input_json and --input_label_h5")
    ap.add_argument("--input_att_ext", default=".npz", choices=[".npz", ".npy"], help="file type of a feature directory")
    ap.add_argument("--input_json", default="", help="the preprocessing's json: images[*]['id'] and ['split']; image i = image i of the label file")
    ap.add_argument("--norm_att_feat", type=int, default=0, choices=[0, 1], help="1: every region divided by its L2 norm (dataloader.py:475-476), on the device")
    ap.add_argument("--train_only", type=int, default=0, choices=[0, 1], help="1: 'restval' images stay out of the train split (dataloader.py:177)")
    ap.add_argument("--feeder_workers", type=int, default=4, help="reader threads of the feature files (at most 16)")
    ap.add_argument("--self_critical_after", type=int, default=-1, help="iteration from which the self-critical step replaces the XE step (-1: never)")
    ap.add_argument("--train_sample_n", type=int, default=5)
    ap.add_argument("--cached_tokens", default=None, help="document-frequency pickle of the CIDEr-D reward (scripts/prepro_ngrams.py): a path, or a name "
                    "for data/<name>.p (opts.py: coco-train-idxs); without such a file the self-critical step scores with a token-overlap stand-in")
    ap.add_argument("--scheduled_sampling_start", type=int, default=None, help="epoch from which ss_prob rises (opts.py:153-160; -1: never, the shipped configs)")
    ap.add_argument("--drop_worst_after", type=int, default=None, help="epoch from which a step keeps the best (1 - drop_worst_rate) captions (opts.py:165-168, "
                    "tools/train.py:186-189, 216-220; -1: never, the shipped configs)")
    ap.add_argument("--iters_per_epoch", type=int, default=1000, help="the synthetic stream has no epochs of its own: iterations that count as one")
    ap.add_argument("--val_images_use", type=int, default=0, help="images of the validation pass at every save_checkpoint_every iterations (tools/train.py:296-363): the last "
                    "N images of --input_label_h5, kept out of the training draws, or N synthetic images from fixed seeds; 0: no validation")
    ap.add_argument("--language_eval", type=int, default=0, choices=[0, 1], help="1: BLEU-1..4, ROUGE-L and CIDEr of the validation captions on the device "
                    "(boficap_amd.lang_eval); the best checkpoint is then chosen by CIDEr instead of the validation loss")
    ap.add_argument("--save_history_ckpt", action="store_true", help="also keep every validated checkpoint as model-<iteration>.pth")
    args = ap.parse_args()
    if bool(args.input_att_dir) != bool(args.input_json):
        ap.error("--input_att_dir and --input_json go together: the feature files are keyed by the json's image ids")
    if args.input_att_dir and args.self_critical_after >= 0:
        ap.error("--self_critical_after is not supported with --input_att_dir: the self-critical step has not been validated on feature files "
                 "(ragged, masked batches); train the XE phase on them, or the self-critical phase on synthetic features")
    if args.input_att_dir and not args.input_label_h5:
        ap.error("--input_att_dir needs the captions of its images: --input_label_h5")

    import numpy as np

    import captioning.models as models
    from boficap_amd import checkpoint as ck, dp, weights as W
    from boficap_amd.collate import synthetic_training_batch
    from boficap_amd.config import FULL, TINY
    from boficap_amd.trainer import XETrainer

    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(dev)                                   # before the process group: RCCL binds to the current device
    rank, local_rank, world = dp.init_from_env("nccl")
    opt = (TINY if args.tiny else FULL).to_opt()
    if args.cfg:
        for k, v in ck.load_yaml_with_base(args.cfg).items():
            setattr(opt, k, v)
    for k in ("batch_size", "seq_per_img"):
        if getattr(args, k) is not None:
            setattr(opt, k, getattr(args, k))
    opt.batch_size, opt.seq_per_img = getattr(opt, "batch_size", 10), getattr(opt, "seq_per_img", 5)
    # the dropout streams of the ranks differ (nn.DataParallel replicas draw from per-device generators); the weights' seed does not
    opt.seed = args.seed + 1000003 * rank
    opt.id, opt.checkpoint_path = args.id, args.checkpoint_path
    opt.bofi_train_dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    if not hasattr(opt, "vocab"):
        opt.vocab = {str(i): f"w{i}" for i in range(1, getattr(opt, "vocab_size", 9487) + 1)}
    torch.manual_seed(args.seed)                                 # same initial weights on every rank (train.py:29-37)
    model = models.setup(opt)
    if args.start_from:
        model.load_state_dict(torch.load(os.path.join(args.start_from, "model.pth"), map_location="cpu"), strict=True)
    model.to(dev).train()
    trainer = XETrainer(model, opt, graph=not args.no_graph)
    infos, histories = ck.new_infos(opt.vocab), {}           # incl. 'loader_state_dict': the reference's resume path indexes it (train.py:125)
    if args.start_from:
        if os.path.exists(os.path.join(args.start_from, "optimizer.pth")):
            trainer.load_state_dict(torch.load(os.path.join(args.start_from, "optimizer.pth"), map_location="cpu", weights_only=False))
        saved, histories = ck.load_infos(args.start_from, args.id)
        if saved:
            if "opt" in saved:
                ck.check_resume_opts(saved["opt"], opt)            # tools/train.py:66-68
            infos.update({k: saved[k] for k in ("iter", "epoch", "best_val_score") if k in saved})
    for k in ("loss_history", "lr_history", "ss_prob_history", "val_result_history"):
        histories.setdefault(k, {})
    cfg = model.cfg
    store = None
    if args.input_label_h5:
        from boficap_amd.data import LabelStore
        src = args.input_label_h5 if args.input_label_h5.endswith((".h5", ".hdf5")) else dict(np.load(args.input_label_h5))
        store = LabelStore(src, pad_idx=cfg.pad_idx, bos_idx=cfg.bos_idx, eos_idx=cfg.eos_idx, len_idx=cfg.len_idx)
    n_val, val = max(0, args.val_images_use), None
    att_store, train_ix, val_ix = None, None, None
    if args.input_att_dir:
        from boficap_amd.features import ImageIndex, RegionFeeder, RegionSource, RegionStore, att_masks_of
        index = ImageIndex(args.input_json, args.train_only)
        if len(index) != store.num_images:
            raise SystemExit(f"{args.input_json} lists {len(index)} images, the label file {store.num_images}")
        train_ix, val_ix = index.split_ix["train"], index.split_ix["val"][:n_val]
        if not train_ix or len(val_ix) < n_val:
            raise SystemExit(f"{args.input_json}: {len(train_ix)} training images, {len(index.split_ix['val'])} validation images (--val_images_use {n_val})")
        att_store = RegionStore(args.input_att_dir, args.input_att_ext)
    elif store is not None and n_val >= store.num_images:
        raise SystemExit(f"--val_images_use {n_val} leaves no training image of the label file's {store.num_images}")
    if n_val and rank == 0:                                      # the validation set, fixed for the run; its references are packed on first use and kept
        from boficap_amd import eval_utils
        if att_store is not None:
            val = {"labels": store, "ixs": list(val_ix), "feats": RegionSource(att_store, index.keys(val_ix), bool(args.norm_att_feat))}
        elif store is not None:
            val = {"labels": store, "ixs": list(range(store.num_images - n_val, store.num_images)),
                   "feats": W.synthetic_att_feats(n_val, 36, cfg.att_feat_size, seed=args.seed + 977)}
        else:
            labels = eval_utils.SyntheticLabels(cfg, n_val, opt.seq_per_img, seed=args.seed + 977)
            val = {"labels": labels, "ixs": None, "feats": labels.feats}
        val["kwargs"] = {"batch_size": min(n_val, model.max_batch), "seq_per_img": opt.seq_per_img, "language_eval": args.language_eval,
                         "image_ixs": val["ixs"], "vocab": opt.vocab, "lang_eval": None}

    def validate_and_save(iteration):
        """tools/train.py:296-363: the validation pass on rank 0 (the other ranks wait), its history entry, the checkpoint and the best one."""
        if n_val and rank == 0:
            from boficap_amd import eval_utils
            kw = val["kwargs"]
            sa_kw = dict(kw, inference_mode="SAIC", verbose_loss=0)
            _, _, sa_stats = eval_utils.eval_split(model, val["feats"], val["labels"], sa_kw)
            kw["lang_eval"] = sa_kw["lang_eval"]                # the references' records: built by the run's first pass, kept from then on
            val_loss, pred, stats = eval_utils.eval_split(model, val["feats"], val["labels"], dict(kw, inference_mode="NAIC"))
            line = " ".join(f"{k} {v:.4f}" for k, v in (stats or {}).items())
            line += "".join(f" SA_{k} {v:.4f}" for k, v in (sa_stats or {}).items())
            print(f"iter {iteration} validation loss {val_loss:.4f} {line}".rstrip(), flush=True)
            histories["val_result_history"][iteration] = {"loss": val_loss, "lang_stats": stats, "predictions": pred}
            current = stats["CIDEr"] if args.language_eval == 1 else -val_loss
            best = infos.get("best_val_score")
            best_flag = best is None or current > best
            infos["best_val_score"] = current if best_flag else best
            if args.checkpoint_path:
                infos["opt"] = ck.resume_opt(opt)
                ck.save_checkpoint(opt, model, infos, trainer, histories)
                if args.save_history_ckpt:
                    ck.save_checkpoint(opt, model, infos, trainer, append=str(iteration))
                if best_flag:
                    ck.save_checkpoint(opt, model, infos, trainer, append="best")
        elif args.checkpoint_path and rank == 0:
            infos["opt"] = ck.resume_opt(opt)
            ck.save_checkpoint(opt, model, infos, trainer, histories)
        if n_val and world > 1:
            torch.distributed.barrier()

    if rank == 0:
        print(f"{type(model).__name__}: {trainer.bucket.numel} parameters in one bucket, {world} rank(s), "
              f"{opt.batch_size} images x {opt.seq_per_img} captions per rank and step, GEMM operands {args.dtype}", flush=True)

    from boficap_amd import loss_wrapper as LW
    scorer = None
    if args.self_critical_after >= 0:
        from boficap_amd.cider import CiderD, resolve_df
        if args.cached_tokens is not None:
            opt.cached_tokens = args.cached_tokens
        df = resolve_df(getattr(opt, "cached_tokens", "coco-train-idxs"))
        cw, bw = float(getattr(opt, "cider_reward_weight", 1)), float(getattr(opt, "bleu_reward_weight", 0) or 0)
        if float(getattr(opt, "self_cider_reward_weight", 0) or 0) > 0:
            # the self-CIDEr term (boficap_amd.diversity) enters the advantage in LossWrapper's StructureLosses; XETrainer.rl_step's captured
            # gradient pass has no input for it, and training on without the term would be a different objective
            raise SystemExit("self_cider_reward_weight > 0: XETrainer.rl_step does not take the self-CIDEr reward term; "
                             "boficap_amd.loss_wrapper.LossWrapper (StructureLosses) does, with the df file of cached_tokens")
        if bw > 0 and (df is not None or not cw > 0):          # get_scores' two terms in one scorer, its weights inside
            from boficap_amd.rewards import RewardScorer
            scorer = RewardScorer(df=df if cw > 0 else None, cider_weight=cw, bleu_weight=bw, device=dev)
            what = f"{cw:g} x CIDEr-D (document frequencies of {df}) + {bw:g} x BLEU-4" if cw > 0 else f"{bw:g} x BLEU-4"
        elif not bw > 0 and df is not None:
            scorer = CiderD(df=df, device=dev)
            what = "CIDEr-D, document frequencies of " + df
        else:
            what = "token-overlap stand-in (no cached_tokens file)"
        if rank == 0:
            print(f"self-critical reward: {what}", flush=True)
    t0, first = time.time(), trainer._step

    def step_seed(it):                                           # a different shard per rank and step (the loader's role, dataloader.py:550-556)
        return (it * world + rank) * 7919 + args.seed

    def step_images(it):
        """The label-file images of step ``it`` and the generator that goes on to draw their captions: a pure function of the iteration number."""
        rng = np.random.default_rng(step_seed(it))
        if train_ix is None:
            return rng.integers(0, store.num_images - n_val, opt.batch_size), rng
        return [train_ix[int(d)] for d in rng.integers(0, len(train_ix), opt.batch_size)], rng

    feed = None
    if att_store is not None:                                    # the steps' features, read and staged ragged by threads that run a few steps ahead
        feed = iter(RegionFeeder(att_store, (index.keys(step_images(it)[0]) for it in range(first, first + args.max_iters)), workers=args.feeder_workers,
                                 norm_att_feat=bool(args.norm_att_feat)))

    def step_features(seed):
        """(att_feats float32 [B, R, F], att_masks [B, R] or None) of this step on the device."""
        if feed is None:
            return torch.from_numpy(W.synthetic_att_feats(opt.batch_size, 36, cfg.att_feat_size, seed=seed)).to(dev), None
        att, att_len = next(feed).to_device(out_dtype=torch.float32)
        return att, att_masks_of(att_len, att.size(1))

    for it in range(first, first + args.max_iters):
        seed = step_seed(it)
        gts = None
        if store is None:
            host_batch = synthetic_training_batch(cfg, opt.batch_size, opt.seq_per_img, seed=seed)
        else:
            ixs, rng = step_images(it)
            host_batch = store.batch(ixs, opt.seq_per_img, rng)
            gts = host_batch.pop("gts")
        ss_start = args.scheduled_sampling_start if args.scheduled_sampling_start is not None else getattr(opt, "scheduled_sampling_start", -1)
        epoch = it // max(1, args.iters_per_epoch)
        infos["epoch"] = epoch
        if ss_start >= 0 and epoch >= ss_start:                 # scheduled sampling probability (tools/train.py:159-162)
            frac = (epoch - ss_start) // getattr(opt, "scheduled_sampling_increase_every", 5) + 1
            opt.ss_prob = min(getattr(opt, "scheduled_sampling_increase_prob", 0.05) * frac, getattr(opt, "scheduled_sampling_max_prob", 0.25))
            model.ss_prob = opt.ss_prob
        if 0 <= args.self_critical_after <= it:                 # struc_flag (tools/train.py:181-185)
            att, _ = step_features(seed)                         # (synthetic features: feature files are refused with --self_critical_after)
            refs = gts if gts is not None else [host_batch["labels"][b, :, 1:-1] for b in range(opt.batch_size)]
            n = args.train_sample_n

            def score(seq, refs=refs, n=n):
                if LW._SCORER["fn"] is not None:
                    return LW._SCORER["fn"](refs, seq)
                out = torch.zeros(seq.shape[0])                  # stand-in: best token overlap with one of the image's captions
                for i, s_ in enumerate(seq.numpy()):
                    toks = set(int(t) for t in s_ if t > 0)
                    out[i] = max((len(toks & set(int(t) for t in r if t > 0)) / max(1, len(toks)) for r in np.asarray(refs[i // n])), default=0.0)
                return out
            if LW._SCORER["fn"] is None and scorer is not None:  # get_scores (rewards.py:86-131) on the device
                score = scorer.bind(refs, n, weight=cw) if isinstance(scorer, CiderD) else scorer.bind(refs, n)
            loss, rs, rn = trainer.rl_step(att, None, score, sample_n=n)
            if (it + 1) % args.losses_log_every == 0 or it == first:
                if rank == 0:
                    print(f"iter {it + 1} lr {trainer.rate():.3e} struc_loss {float(loss):.4f} reward SAIC {float(rs):.4f} NAIC {float(rn):.4f} "
                          f"{(time.time() - t0) / (it + 1 - first):.3f} s/it", flush=True)
                histories["loss_history"][it + 1] = float(loss)
            infos["iter"] = it + 1
            if n_val and args.save_checkpoint_every and (it + 1) % args.save_checkpoint_every == 0:
                validate_and_save(it + 1)
            continue
        batch = {k: torch.from_numpy(v).to(dev) for k, v in host_batch.items()}
        batch["max_phrase_num"] = int(host_batch["phrase_num"].max())
        batch["max_tokens"] = int((host_batch["phrase_length"].sum(-1) - 1).max())
        batch["att_feats"], att_masks = step_features(seed)
        if att_masks is not None:
            batch["att_masks"] = att_masks
        batch = trainer.add_token_rows(batch, host_batch)
        glat_p = args.unmasked_rate_start if args.glancing_token else -1.0          # train.py:165-170
        dw_after = args.drop_worst_after if args.drop_worst_after is not None else getattr(opt, "drop_worst_after", -1)
        drop_worst = dw_after != -1 and epoch >= dw_after                         # train.py:186-189
        try:
            loss, parts = trainer.step(batch, glat_p, drop_worst)
        except FloatingPointError as e:                          # scheduled sampling on a model whose SA bounding step opens no phrase for
            if not model.ss_prob > 0:                            # some caption: the reference crashes there (TransformerModel.py:2103-2105);
                raise                                            # this batch is stepped teacher-forced instead
            if rank == 0:
                print(f"iter {it + 1}: {e}; teacher-forced step for this batch", flush=True)
            keep, model.ss_prob = model.ss_prob, 0.0
            loss, parts = trainer.step(batch, glat_p, drop_worst)
            model.ss_prob = keep
        if (it + 1) % args.losses_log_every == 0 or it == 0:
            mean_loss = dp.reduce_scalar(float(loss), "sum", device=dev) / world
            if rank == 0:
                names = ("sa_len", "sa_tok", "sa_syn", "na_len", "na_tok", "na_syn")
                detail = " ".join(f"{n}={float(p):.3f}" for n, p in zip(names, parts))
                print(f"iter {it + 1} lr {trainer.rate():.3e} train_loss {mean_loss:.4f} ({detail}) "
                      f"{(time.time() - t0) / (it + 1 - first):.3f} s/it", flush=True)
            histories["loss_history"][it + 1] = mean_loss         # tools/train.py:262-266
            histories["lr_history"][it + 1] = trainer.rate()
            histories["ss_prob_history"][it + 1] = model.ss_prob
        infos["iter"] = it + 1                                   # tools/train.py:292-294
        if args.save_checkpoint_every and (it + 1) % args.save_checkpoint_every == 0 and (args.checkpoint_path or n_val):
            validate_and_save(it + 1)
    if feed is not None:
        feed.close()                                             # (ends the feeder's threads)
    if args.checkpoint_path and rank == 0:
        infos["opt"] = ck.resume_opt(opt)                     # plain values, every option of the reference's resume check present
        ck.save_checkpoint(opt, model, infos, trainer, histories)
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
