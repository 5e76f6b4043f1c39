"""Host-side mirror of the reference's ``LossWrapper`` for ``train_mode: UIC`` (captioning/modules/loss_wrapper.py:181-244):
same constructor, same ``forward`` signature, same keys in the returned dict, so that ``tools/train.py``'s
``lw_model(fc, att, labels, masks, att_masks, gts, gt_indices, sc_flag, struc_flag, drop_worst_flag, phrase, ...)`` call
(tools/train.py:212-213) works on the drop-in model.  The arithmetic is the HIP path's: ``model(..., mode='forward')`` /
``mode='sample'`` run on libboficap_hip.so, the criteria are the fused kernels and index bookkeeping of ``boficap_amd.xe``.

XE branch (struc_flag False): pinned to the reference by tests/golden/tiny_loss_wrapper_xe (the reference's LossWrapper
around the reference model).  RL branch (struc_flag True): its loss arithmetic is pinned by tests/golden/tiny_rl_loss
(StructureLosses 'new_self_critical' and the rl_kl term with injected samples and scores) and tests/golden/tiny_structure_losses (the other
structure_loss_types); the caption scorer itself
(``get_scores``, captioning/utils/rewards.py:86-131) is ``opt.bofi_score_fn(gts, seq) -> [N] floats`` or one installed with ``set_scorer`` if
given, else the device scorer of ``device_scorer``: CIDEr-D of ``opt.cached_tokens`` (boficap_amd.cider), and with ``opt.bleu_reward_weight`` > 0
the weighted sum with BLEU-4 (boficap_amd.rewards).  With ``opt.self_cider_reward_weight`` > 0 and 'new_self_critical' the self-CIDEr diversity
of every image's samples (boficap_amd.diversity, the df file of ``opt.cached_tokens``) is added to the advantage, whichever scorer gave the reward.

RL branch, the estimator (round 6): the reference samples with the autograd tape running (and dropout active) and
differentiates that same pass (loss_wrapper.py:193-209).  In train mode this class does the same by default, as ``XETrainer.rl_step`` does
since round 5 (``reference_estimator_pass`` below): every token of both branches is drawn from the TRAINING forward's rows under
the step's counter-based dropout masks, phrase by phrase, and the returned log-probs are that forward once more with the tape -- at the
drawn tokens they equal the rows they were drawn from bit for bit (``LossWrapper.last_rl["reference_gap"]`` = 0.0).
``opt.bofi_rl_reference_estimator = False`` keeps the fast form of rounds 1-5: samples from the decode engine (no dropout, no tape),
``xe.sampled_logprobs`` recomputes their log-probs with the tape (with dropout): a different estimator, ~2x cheaper.  In eval mode the two
coincide (no dropout anywhere) and the fast form runs.
"""
from __future__ import annotations

import os

import torch

from . import cider, hip, rl_draws, xe

_SCORER = {"fn": None}


def set_scorer(fn) -> None:
    """Install the caption scorer of the RL branch: ``fn(data_gts, gen_result int64 [N, S] on the host) -> [N]`` floats
    (the role of get_scores, captioning/utils/rewards.py:86-131)."""
    _SCORER["fn"] = fn


_DEVICE_SCORER: dict = {}


def device_scorer(opt):
    """The device scorer of get_scores (rewards.py:86-131) for ``opt``, built once per df file and weights as init_scorer does (rewards.py:25-31):
    with ``bleu_reward_weight`` 0 the CIDEr-D scorer of ``opt.cached_tokens`` (boficap_amd.cider.CiderD, weighted at the call), else the
    combined cider_reward_weight * CIDEr-D + bleu_reward_weight * BLEU-4 (boficap_amd.rewards.RewardScorer, weights inside; a df file is
    needed only if cider_reward_weight > 0).  Raises where no scorer can be built: no df file for a CIDEr-D term, or neither weight > 0."""
    bw = float(getattr(opt, "bleu_reward_weight", 0) or 0)
    cw = float(getattr(opt, "cider_reward_weight", 1))
    path = cider.resolve_df(getattr(opt, "cached_tokens", "coco-train-idxs"))
    if bw > 0:
        from .rewards import RewardScorer
        if cw > 0 and path is None:
            raise hip.BofiHipError("no caption scorer: the CIDEr-D term needs a document-frequency file for opt.cached_tokens (data/<cached_tokens>.p "
                                   "of scripts/prepro_ngrams.py); pass opt.bofi_score_fn or call boficap_amd.loss_wrapper.set_scorer")
        path = path if cw > 0 else None
        key = ("reward", os.path.abspath(path) if path not in (None, "corpus") else path, cw, bw, torch.cuda.current_device())
        if key not in _DEVICE_SCORER:
            _DEVICE_SCORER[key] = RewardScorer(df=path, cider_weight=cw, bleu_weight=bw)
        return _DEVICE_SCORER[key]
    if path is None or not cw > 0:
        raise hip.BofiHipError("no caption scorer: no document-frequency file for opt.cached_tokens (data/<cached_tokens>.p of scripts/prepro_ngrams.py) "
                               "and no scorer installed; pass opt.bofi_score_fn or call boficap_amd.loss_wrapper.set_scorer")
    key = (os.path.abspath(path) if path != "corpus" else path, torch.cuda.current_device())
    if key not in _DEVICE_SCORER:
        _DEVICE_SCORER[key] = cider.CiderD(df=path)
    return _DEVICE_SCORER[key]


def reference_estimator_pass(model, att_feats, att_masks, sample_n: int, temperature: float, seed: int):
    """loss_wrapper.py:193-209 (``model(..., mode='sample')`` twice in train mode with the tape, then the loss on THOSE log-probs) on this build's training
    forward, without a trainer (the caller owns backward and the optimiser): ``rl_draws.draw_pass`` -- the one draw pass, ``XETrainer._rl_reference_step``'s
    too -- draws every token of both branches from eager tape-free training forwards under ``seed``, then the same forward once more WITH the tape:
    counter-based dropout masks (seed, site, element) make it the same rows bit for bit.
    Returns (saic log-probs [N, S, V] with grad, naic log-probs, saic dict, naic dict, gap) -- ``gap``: max |tape row - drawn row| at the drawn tokens (0.0)."""
    cfg, P = model.cfg, xe.Params(model)
    shared: dict = {}                                             # the encoder's memory and the cross K|V: the same tensors in every tape-free forward of this step

    def rows_of(prep, reuse=None):
        return xe.sampled_logprobs_prepared(P, cfg, att_feats, att_masks, prep, sample_n=sample_n, training=True, seed=seed, compute_dtype=model.train_dtype, reuse=reuse)

    d = rl_draws.draw_pass(model, rl_draws.naic_layout(model, att_feats, att_masks, sample_n), temperature,
                           lambda layout, first: rows_of(rl_draws.prepared(cfg, layout), shared), draw_base=seed + 0x5EED0000)
    lp_saic, lp_naic = rows_of(d.prep)                            # the gradient pass: the same rows, with the tape
    with torch.no_grad():
        gap = rl_draws.drawn_gap(rl_draws.picked(lp_saic, d.seq_s), rl_draws.picked(lp_naic, d.seq_n), d)
    saic = {"seq": d.seq_s, "phrase_num": d.out["phrase_num"], "phrase_length": d.out["phrase_length"], "phrase_syn": d.out["phrase_syn"]}
    return lp_saic, lp_naic, saic, d.naic, {"reference_gap": gap, "training_forwards": d.passes + 1}


class LanguageModelCriterion_UIC(torch.nn.Module):
    """captioning/modules/losses.py:315-369: (loss, SA length, SA phrase, SA syn, NA length, NA phrase, NA syn); with reduction
    'none' the loss is one value per caption and the six parts are None, as in the reference (:357-361)."""

    def forward(self, sa_len, sa_syn, sa_tok, na_len, na_syn, na_tok, phrase_num, phrase_length, phrase_syn, labels, reduction="mean", self_dis=False):
        loss, parts = xe.criterion_uic((sa_len, sa_syn, sa_tok, na_len, na_syn, na_tok), phrase_num, phrase_length, phrase_syn, labels,
                                       reduction=reduction, self_dis=self_dis)
        return (loss, *(parts if parts is not None else [None] * 6))


class StructureLosses(torch.nn.Module):
    """captioning/modules/losses.py:29-179: every ``structure_loss_type`` (configs/uic_sd_kd100_sd_nscl.yml uses 'new_self_critical'),
    the entropy reward, reduction 'none' (xe.structure_loss) and the self-CIDEr reward term of 'new_self_critical' (:167-171): weight x the
    self-CIDEr diversity of the image's samples (``self_cider_term``), added to every sample's advantage after the baseline subtraction."""

    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        self.loss_type = getattr(opt, "structure_loss_type", "seqnll")

    def self_cider_term(self, input, seq, n):
        """losses.py:167-171: ``self_cider_reward_weight`` x get_self_cider_scores as [B, 1] in ``input``'s dtype, on the device (no host
        copy, no sync); None unless the weight is above 0 and the type is 'new_self_critical' (the other types ignore the weight).  An image
        whose samples hold no n-gram of non-zero weight (e.g. every sample the id 0 alone, with (0) in every document of the df file) scores
        NaN, as the reference's formula does, and so do the advantage and the batch's loss."""
        w = float(getattr(self.opt, "self_cider_reward_weight", 0) or 0)
        if not w > 0 or self.loss_type != "new_self_critical":
            return None
        from .diversity import self_cider_scorer
        score = self_cider_scorer(self.opt, seq.device if seq.is_cuda else None).score(seq.detach().to(input.device), n)
        return w * score.to(input.dtype).view(-1, 1)              # (the reference casts the scores first, then weighs them)

    def forward(self, input, seq, data_gts, reduction="mean"):
        n = input.size(0) // len(data_gts)
        assert n == self.opt.train_sample_n, n                   # losses.py:45
        fn = getattr(self.opt, "bofi_score_fn", None) or _SCORER["fn"]
        if fn is None:                                            # get_scores (rewards.py:86-131) on the device: CIDEr-D of the df file opt.cached_tokens
            sc = device_scorer(self.opt)                          # (+ BLEU-4 with bleu_reward_weight > 0: the weights live in that scorer)
            if isinstance(sc, cider.CiderD):
                scores = sc.score(data_gts, seq.detach(), n, weight=float(getattr(self.opt, "cider_reward_weight", 1)))
            else:
                scores = sc.score(data_gts, seq.detach(), n)
        else:
            scores = fn(data_gts, seq.detach().cpu())
        loss, reward = xe.structure_loss(self.loss_type, input, seq, scores, n, reduction=reduction,
                                         entropy_reward_weight=float(getattr(self.opt, "entropy_reward_weight", 0) or 0),
                                         extra_advantage=self.self_cider_term(input, seq, n))
        return {"loss": loss, "reward": reward}


class LossWrapper(torch.nn.Module):
    def __init__(self, model, opt):
        super().__init__()
        self.opt = opt
        self.model = model
        self.train_mode = getattr(opt, "train_mode", "AIC")
        self.self_dis = getattr(opt, "self_dis", False)
        self.rl_kl = getattr(opt, "rl_kl", False)
        if self.train_mode != "UIC":
            raise NotImplementedError(f"train_mode {self.train_mode!r}: the unified bound+fill model (UIC) is built")
        self.crit = LanguageModelCriterion_UIC()
        self.struc_crit = StructureLosses(opt)
        self.last_rl = None                                       # diagnostics of the last struc_flag step: {"reference_gap", "training_forwards"}

    def forward(self, fc_feats, att_feats, labels, masks, att_masks, gts, gt_indices, sc_flag, struc_flag, drop_worst_flag, phrase=None,
                phrase_num=None, phrase_length=None, phrase_syn=None, extend_phrase_syn_seq=None, extend_phrase_seq=None,
                extend_phrase_seq_mask=None, glat_p=0.3):
        opt = self.opt
        reduction = "none" if drop_worst_flag else "mean"         # loss_wrapper.py:39: the caller keeps the best captions (tools/train.py:216-220)
        out = {}
        xe_args = (fc_feats, att_feats, labels, att_masks, phrase_num, phrase_length, phrase_syn, extend_phrase_syn_seq, extend_phrase_seq,
                   extend_phrase_seq_mask)
        if not struc_flag:                                        # loss_wrapper.py:231-244
            outs = self.model(*xe_args, glat_p)
            loss, *parts = self.crit(*outs, phrase_num, phrase_length, phrase_syn, labels, reduction=reduction, self_dis=self.self_dis)
            for k, v in zip(("SA_length_loss", "SA_phrase_loss", "SA_syn_loss", "NA_length_loss", "NA_phrase_loss", "NA_syn_loss"), parts):
                out[k] = v
            out["loss"] = loss
            return out
        # ---- struc_flag (loss_wrapper.py:181-230)
        w = float(opt.structure_loss_weight)
        if w < 1:
            outs = self.model(*xe_args)
            lm_loss = self.crit(*outs, phrase_num, phrase_length, phrase_syn, labels)[0]
        else:
            lm_loss = torch.tensor(0).type_as(fc_feats)
        if w > 0:
            n = int(opt.train_sample_n)
            sopt = {"sample_method": opt.train_sample_method, "beam_size": getattr(opt, "train_beam_size", 1), "output_logsoftmax": 1, "sample_n": n}
            ks = ("seq", "seq_logprob", "phrase_num", "phrase_length", "phrase_syn")
            self.model._step = getattr(self.model, "_step", 0) + 1
            seed = (int(getattr(opt, "seed", 0)) << 32) + self.model._step if self.model.training else None
            if self.model.training and getattr(opt, "bofi_rl_reference_estimator", True) and opt.train_sample_method == "sample":
                # the reference's estimator (loss_wrapper.py:193-209): tokens drawn from the rows this pass differentiates
                lp_s, lp_n, saic, naic, self.last_rl = reference_estimator_pass(self.model, att_feats, att_masks, n, 1.0, seed)      # (temperature 1.0: the reference's sample opts carry none, loss_wrapper.py:194-199)
            else:
                was_training = self.model.training
                self.model.eval()                                 # the sampler is the decode engine (no dropout, no tape)
                with torch.no_grad():
                    saic = dict(zip(ks, self.model(fc_feats, att_feats, att_masks, opt=dict(sopt, train_mode="SAIC"), mode="sample")[:5]))
                    naic = dict(zip(ks, self.model(fc_feats, att_feats, att_masks, opt=dict(sopt, train_mode="NAIC"), mode="sample")[:5]))
                self.model.train(was_training)
                lp_s, lp_n = xe.sampled_logprobs(xe.Params(self.model), self.model.cfg, att_feats, att_masks, saic, naic, sample_n=n,
                                                 strict_q1=self.model.strict_reference, training=self.model.training, seed=seed,
                                                 compute_dtype=self.model.train_dtype)
                self.last_rl = {"reference_gap": None, "training_forwards": 1}
            gts = [gts[_] for _ in gt_indices.tolist()]
            s_loss = self.struc_crit(lp_s, saic["seq"], gts)
            n_loss = self.struc_crit(lp_n, naic["seq"], gts)
            struc_loss = {"loss": s_loss["loss"] + n_loss["loss"], "reward": s_loss["reward"] + n_loss["reward"]}
            loss = ((1 - w) * lm_loss + w * s_loss["loss"]) + ((1 - w) * lm_loss + w * n_loss["loss"])
            if self.rl_kl:                                        # :216-222
                # positions the SAIC sample never emitted hold zero rows in the reference's seq_logprobs (TM:1883); they are
                # masked by (SAIC_seq > 0) in the KL term, so the re-forwarded rows there do not matter
                loss = loss + xe.rl_kl_term(lp_n, lp_s, saic["seq"])
        else:
            raise NotImplementedError("structure_loss_weight 0 under struc_flag leaves the reference's own code with an undefined variable (:213)")
        out["lm_loss"] = lm_loss
        out["struc_loss"] = struc_loss["loss"]
        out["reward"] = struc_loss["reward"]
        out["loss"] = loss
        return out
