"""Does a change to the training plumbing leave every form of the XE / self-critical step as it was?

    python dev/step_equivalence.py run --tree PARENT_CHECKOUT --out A1        # the parent commit (built), twice
    python dev/step_equivalence.py run --tree PARENT_CHECKOUT --out A2
    python dev/step_equivalence.py run --out B                                 # this tree
    python dev/step_equivalence.py compare A1 A2 B --table profiles/rNN_equivalence.txt

``run`` (one process per tree; needs the GPU): TINY weights from a seed, fixed synthetic batches, model.train() under a fixed opt.seed -- the
dropout masks are counter-based by (seed, site, element), so a changed launch order changes the loss.  Per case a few forward + backward
calls on unchanged weights (XE: forward_backward; self-critical: rl_step at learning rate 0, and LossWrapper's struc_flag branch + backward),
the losses and loss parts of every call as hex floats -- for the reference-estimator forms also a sha256 of the call's drawn ids and layouts, compared
like a loss -- (cases.json) and the gradient bucket (LossWrapper: the parameters' gradients) after the last call (<case>.pt).  ``compare``: losses must be bit-equal; gradients go through
float atomics, so the parent against itself gives the noise (max and mean |dgrad| per case) and the branch against the parent may show at
most twice that.  Exit status 1 if a case misses either."""
import argparse
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTOR = 2.0          # the fluctuation of a maximum over one more sample of the same noise; a changed computation is orders above it


def cases():
    """(name, what the case needs).  forms: dense = the loader's batch, compact / unpadded / paired = add_token_rows of trainers built so."""
    out = []
    for dt in ("f32", "bf16"):
        for graph in (False, True):
            for form in ("dense", "compact", "unpadded", "paired"):
                out.append((f"xe {form} {dt} {'graph' if graph else 'eager'}", dict(form=form, dtype=dt, graph=graph)))
    for form, dt, graph in (("dense", "f32", False), ("unpadded", "f32", False), ("paired", "f32", False), ("paired", "bf16", True)):
        out.append((f"xe {form} {dt} {'graph' if graph else 'eager'} glat 0.5", dict(form=form, dtype=dt, graph=graph, glat_p=0.5)))
    out.append(("xe unpadded bf16 eager side-streams", dict(form="unpadded", dtype="bf16", graph=False, streams=True)))
    out.append(("xe paired bf16 eager dw-aside 6", dict(form="paired", dtype="bf16", graph=False, opt=dict(bofi_dw_every=6))))
    for dt in ("f32", "bf16"):
        out.append((f"xe paired {dt} graph drop_worst", dict(form="paired", dtype=dt, graph=True, drop_worst=True)))
        out.append((f"xe paired {dt} graph self_dis", dict(form="paired", dtype=dt, graph=True, opt=dict(self_dis=True))))
        out.append((f"xe paired {dt} graph scheduled-sampling 0.25", dict(form="paired", dtype=dt, graph=True, ss_prob=0.25)))
        out.append((f"xe paired {dt} graph N_len 2", dict(form="paired", dtype=dt, graph=True, n_len=2)))
    for ref in (True, False):
        for dt, graph in (("f32", False), ("bf16", False), ("bf16", True)):
            out.append((f"rl {'reference' if ref else 'fast'}-estimator {dt} {'graph' if graph else 'eager'}", dict(rl=ref, dtype=dt, graph=graph)))
    out.append(("rl reference-estimator f32 eager ragged", dict(rl=True, dtype="f32", graph=False, ragged=True)))
    for dt in ("f32", "bf16"):                                 # LossWrapper's struc_flag branch in train mode: the same draw pass without a trainer
        out.append((f"lw rl reference {dt}", dict(lw=True, dtype=dt, graph=False, opt=dict(
            structure_loss_type="new_self_critical", train_sample_n=3, structure_loss_weight=1, train_sample_method="sample", train_beam_size=1))))
    return out


def _digest(*tensors):
    """sha256 over the tensors' bytes (drawn ids, slot layouts): equal hashes = the same draws."""
    import hashlib
    import torch
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().to(torch.int64).cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def run(tree, out_dir):
    sys.path.insert(0, os.path.abspath(tree))
    import numpy as np
    import torch
    import captioning.models as models
    from boficap_amd import weights as W, xe
    from boficap_amd.collate import synthetic_training_batch
    from boficap_amd.config import TINY, TINY_N2
    from boficap_amd.trainer import XETrainer
    os.makedirs(out_dir, exist_ok=True)
    n_img, calls = 3, 3
    record = {}
    for name, c in cases():
        cfg = TINY_N2 if c.get("n_len") == 2 else TINY
        sd = W.make_state_dict(cfg, seed=0)
        if "rl" in c or "lw" in c or c.get("ss_prob"):
            sd = W.with_len_row_shared(sd, cfg)                # (the semi-autoregressive mode lays out several phrases with these)
        opt = cfg.to_opt()
        opt.seed, opt.noamopt, opt.learning_rate = 7, False, 0.0
        for k, v in c.get("opt", {}).items():
            setattr(opt, k, v)
        model = models.setup(opt)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        model.cuda().train()
        model.train_dtype = torch.bfloat16 if c["dtype"] == "bf16" else torch.float32
        torch.manual_seed(11)
        # (scheduled sampling: a caption whose first sampled slot is empty is left without keys and raises -- images and a batch that have none)
        spi, bseed, aseed = (2, 3, 4) if c.get("ss_prob") else (3, 12, 3)
        att = torch.from_numpy(W.synthetic_att_feats(n_img, 36, cfg.att_feat_size, seed=aseed)).cuda()
        losses, tr = [], None
        if "rl" in c or "lw" in c:
            # (the images of the fixture these weights lay several phrases out on: an image whose samples are all empty gives a NaN loss)
            att = torch.from_numpy(np.load(os.path.join(ROOT, "tests", "golden", "tiny_saic_multi.npz"))["att_feats"]).cuda()
            masks = None
            if c.get("ragged"):
                masks = torch.ones(att.shape[:2], device="cuda"); masks[0, 20:] = 0
        if "lw" in c:
            from boficap_amd.loss_wrapper import LossWrapper
            seen = []                                          # what the scorer hook is handed: the drawn ids of the two branches

            def scorer(gts, seq):
                seen.append(seq)
                return (seq % 7 == 0).float().mean(1)
            model.opt.bofi_score_fn = scorer
            lw = LossWrapper(model, model.opt)
            fc, gts = torch.zeros(att.size(0), 0, device="cuda"), [[np.zeros(3, np.int64)] for _ in range(att.size(0))]
            for _ in range(calls):
                model.zero_grad()
                del seen[:]
                out = lw(fc, att, None, None, masks, gts, torch.arange(att.size(0)), False, True, False)
                out["loss"].backward()
                losses.append([float(out["loss"]).hex()] + [float(x).hex() for x in out["reward"].flatten()] + [_digest(*seen)])
            grad = torch.cat([(torch.zeros_like(p) if p.grad is None else p.grad).detach().flatten().cpu() for p in model.parameters()])
        elif "rl" in c:
            model.opt.bofi_rl_reference_estimator = c["rl"]
            tr = XETrainer(model, opt, graph=c["graph"])
            for _ in range(calls):
                r = tr.rl_step(att, masks, lambda seq: (seq % 7 == 0).float().mean(1), sample_n=3, temperature=1.0)
                losses.append([float(x).hex() for x in r])
                if c["rl"]:                                    # the draws themselves: ids of both branches and the semi-autoregressive layout
                    last = tr._last_rl
                    losses[-1].append(_digest(last["seq_saic"], last["seq_naic"], last["phrase_length_saic"], last["phrase_syn_saic"]))
        else:
            form = c["form"]
            tr = XETrainer(model, opt, graph=c["graph"], unpadded=form != "compact", paired=form == "paired", streams=bool(c.get("streams")))
            hb = synthetic_training_batch(cfg, n_img, spi, seed=bseed)
            batch = {k: torch.from_numpy(v).cuda() for k, v in hb.items()}
            batch["att_feats"] = att
            batch["max_phrase_num"] = int(hb["phrase_num"].max())
            if form != "dense":
                batch = tr.add_token_rows(batch, hb)
            if c.get("ss_prob"):
                model.ss_prob = c["ss_prob"]
                model._ss_draw = random.Random(5).random
            draws = torch.rand(n_img * spi, cfg.seq_length, generator=torch.Generator().manual_seed(9))
            for _ in range(calls):
                if c.get("glat_p") is not None:
                    xe.HINTS["glat_uniform"] = draws
                loss, parts = tr.forward_backward(batch, glat_p=c.get("glat_p", -1.0), drop_worst=bool(c.get("drop_worst")))
                losses.append([float(x).hex() for x in [loss] + list(parts)])
            xe.HINTS.pop("glat_uniform", None)
        torch.cuda.synchronize()                               # (a case that raises ends the run: every case runs on the parent)
        if tr is not None:
            grad = tr.bucket.grad.detach().cpu()
        torch.save(grad, os.path.join(out_dir, name.replace(" ", "_") + ".pt"))
        record[name] = losses
        print(f"{name}: {losses[-1][0]}", flush=True)
        del tr, model
    with open(os.path.join(out_dir, "cases.json"), "w") as f:
        json.dump(record, f, indent=1)


def compare(a1, a2, b, table):
    import torch
    rec = [json.load(open(os.path.join(d, "cases.json"))) for d in (a1, a2, b)]
    grad = lambda d, name: torch.load(os.path.join(d, name.replace(" ", "_") + ".pt")).double()
    lines, bad = [], []
    lines.append("losses: every call's loss and loss parts as hex floats -- parent run 1 | parent run 2 | branch; gradients: |dgrad| of the bucket after the last call")
    lines.append(f"{'case':<52} {'losses p1=p2':>12} {'losses b=p1':>12} {'parent max':>11} {'parent mean':>11} {'branch max':>11} {'branch mean':>11}  verdict")
    detail = []
    for name, _ in cases():
        l1, l2, lb = (r.get(name) for r in rec)
        g1, g2, gb = grad(a1, name), grad(a2, name), grad(b, name)
        pmax, pmean = float((g1 - g2).abs().max()), float((g1 - g2).abs().mean())
        bmax, bmean = float((gb - g1).abs().max()), float((gb - g1).abs().mean())
        ok = l1 == l2 == lb and bmax <= FACTOR * pmax and bmean <= FACTOR * pmean          # (a NaN anywhere fails the case)
        if not ok:
            bad.append(name)
        lines.append(f"{name:<52} {str(l1 == l2):>12} {str(lb == l1):>12} {pmax:11.3e} {pmean:11.3e} {bmax:11.3e} {bmean:11.3e}  {'ok' if ok else 'DIFFERS'}")
        for i, (x, y, z) in enumerate(zip(l1, l2, lb)):
            detail.append(f"{name} call {i + 1}: {' '.join(x)} | {' '.join(y)} | {' '.join(z)}")
    lines.append(f"{len(cases()) - len(bad)} of {len(cases())} cases: losses bit-equal and the branch's gradient differences within {FACTOR:g} x the parent's own"
                 + ("" if not bad else "; NOT: " + ", ".join(bad)))
    text = "\n".join(lines + [""] + detail) + "\n"
    if table:
        with open(table, "w") as f:
            f.write(text)
    print("\n".join(lines))
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("--tree", default=ROOT)
    r.add_argument("--out", required=True)
    k = sub.add_parser("compare")
    k.add_argument("dirs", nargs=3)
    k.add_argument("--table", default=None)
    a = ap.parse_args()
    sys.exit(run(a.tree, a.out) if a.cmd == "run" else compare(*a.dirs, a.table))
