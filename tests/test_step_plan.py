"""trainer.step_plan: which form of the XE step a batch takes (dense, compact, unpadded, paired), decided from the collate's dict
alone -- no device, no model.  One case per branch."""
import pytest
import torch

from boficap_amd import xe
from boficap_amd.config import TINY
from boficap_amd.trainer import XETrainer, step_plan

S = TINY.seq_length
FIELDS = ("max_phrase_num", "max_tokens", "token_rows", "unpadded", "streams", "paired", "pick_labels", "paired_inputs", "split_memory")
SIDE = ["stream 1", "stream 2", "stream 3"]                       # (stands for the trainer's side streams: passed through, never touched)


def _t(*v):
    return torch.tensor(v, dtype=torch.int64)


def _plain():
    return {"att_feats": torch.zeros(2, 3, 4), "labels": torch.zeros(2, 3, S + 2, dtype=torch.int64)}


def _rows(**more):
    return dict(_plain(), max_phrase_num=5, max_tokens=9, token_rows=_t(0, 1, 12), token_labels=_t(7, 8, 9), token_weight=torch.ones(3), **more)


def _unpadded(**more):
    return _rows(row_start=_t(0, 2), row_count=_t(2, 1), row_cap=_t(0, 0, 1), row_pos=_t(0, 1, 0), **more)


def _paired(**more):
    return _unpadded(pair_start=_t(0, 2, 3, 5), pair_count=_t(2, 1, 2, 1), pair_src=_t(0, 1, 2, 0, 1, 2), pair_na=_t(0, 0, 0, 1, 1, 1).bool(),
                     pair_labels=_t(7, 8, 9, 7, 8, 9), pair_w_sa=torch.ones(6), pair_w_na=torch.ones(6), **more)


def _prep():
    return {k: _t(i) for i, k in enumerate(XETrainer._OPT_KEYS) if k.startswith("prep_")}


def _plan(batch, **kw):
    args = dict(glat_p=-1.0, dense=None, scheduled_sampling=False, streams=None, stage2=None)
    args.update(kw)
    plan = step_plan(batch, S, **args)
    assert isinstance(plan, xe.StepPlan)
    return plan


def test_plain_batch_is_the_dense_step():
    plan = _plan(_plain(), streams=SIDE)
    assert all(getattr(plan, f) is None for f in FIELDS) and plan.criterion == "dense"
    assert plan == xe.StepPlan(criterion="dense")


def test_bounds_are_bucketed_and_capped():
    plan = _plan(dict(_plain(), max_phrase_num=5, max_tokens=9))
    assert (plan.max_phrase_num, plan.max_tokens) == (8, 12) and plan.criterion == "dense"
    plan = _plan(dict(_plain(), max_phrase_num=S + 1, max_tokens=S - 1))
    assert (plan.max_phrase_num, plan.max_tokens) == (S + 1, S)          # the multiple of 4 above 21 is 24: capped at seq_length + 1; 19 -> seq_length
    assert all(getattr(plan, f) is None for f in FIELDS[2:])


def test_token_rows_without_max_tokens_is_not_compact():
    b = _rows()
    del b["max_tokens"]
    plan = _plan(b, streams=SIDE)
    assert plan.token_rows is None and plan.max_tokens is None and plan.max_phrase_num == 8 and plan.criterion == "dense"
    assert all(getattr(plan, f) is None for f in FIELDS[2:])


def test_token_rows_with_max_tokens_is_compact():
    b = _rows()
    plan = _plan(b, streams=SIDE)
    assert plan.token_rows is b["token_rows"] and plan.criterion == "compact" and (plan.max_phrase_num, plan.max_tokens) == (8, 12)
    assert all(getattr(plan, f) is None for f in FIELDS[3:])            # (no row_cap: the decoder stays padded, nothing goes on side streams)


def test_row_cap_is_the_unpadded_step_and_the_only_one_with_streams():
    b = _unpadded()
    plan = _plan(b, streams=SIDE)
    assert len(plan.unpadded) == 5 and all(x is b[k] for x, k in zip(plan.unpadded, ("row_start", "row_count", "row_cap", "row_pos")))
    assert plan.unpadded[4] == 256                                      # the granule add_token_rows pads the row list to
    assert plan.streams is SIDE and plan.token_rows is b["token_rows"] and plan.criterion == "compact"
    assert plan.paired is None and plan.pick_labels is None and plan.paired_inputs is None
    assert _plan(b).streams is None


def test_pair_src_is_the_paired_step():
    b = _paired()
    plan = _plan(b, streams=SIDE)
    assert len(plan.paired) == 5 and all(x is b[k] for x, k in zip(plan.paired, ("pair_start", "pair_count", "pair_src", "pair_na")))
    assert plan.paired[4] == 256
    assert plan.pick_labels is b["pair_labels"] and plan.streams is None and plan.criterion == "paired"
    assert plan.unpadded is not None and plan.token_rows is b["token_rows"] and plan.paired_inputs is None
    b = _paired()
    del b["row_cap"]                                                    # (the pair lists index the unpadded rows: nothing without them)
    plan = _plan(b, streams=SIDE)
    assert plan.paired is None and plan.pick_labels is None and plan.unpadded is None and plan.criterion == "compact"


@pytest.mark.parametrize("masks,glat_p,used", [(False, -1.0, True), (True, -1.0, False), (False, 0.5, False), (False, 0.0, False)])
def test_host_prepared_inputs_only_without_masks_and_glancing(masks, glat_p, used):
    prep = _prep()
    b = _paired(**prep, **({"att_masks": torch.ones(2, 3)} if masks else {}))
    plan = _plan(b, glat_p=glat_p)
    assert plan.criterion == "paired" and plan.paired is not None
    if used:
        assert set(plan.paired_inputs) == {k[5:] for k in prep} and all(plan.paired_inputs[k[5:]] is v for k, v in prep.items())
    else:
        assert plan.paired_inputs is None
    assert _plan(_unpadded(**prep)).paired_inputs is None               # (not paired: nobody reads them)


@pytest.mark.parametrize("kw,criterion", [(dict(dense="plain"), "dense"), (dict(dense="drop_worst"), "drop_worst"),
                                          (dict(scheduled_sampling=True), "dense"),
                                          (dict(scheduled_sampling=True, dense="drop_worst"), "drop_worst")])
def test_dense_forms_take_nothing_from_the_batch(kw, criterion):
    for b in (_plain(), _rows(), _unpadded(), _paired(**_prep())):
        plan = _plan(b, streams=SIDE, **kw)
        assert all(getattr(plan, f) is None for f in FIELDS) and plan.criterion == criterion


def test_stage2_dict_is_the_split_memory():
    stage2 = {}
    for b, kw in ((_plain(), {}), (_paired(), {}), (_rows(), dict(scheduled_sampling=True))):
        assert _plan(b, stage2=stage2, **kw).split_memory is stage2
    assert _plan(_paired()).split_memory is None
