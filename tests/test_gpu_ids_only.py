"""BOFI_FLAG_IDS_ONLY at the engine level (decode_naic(ids_only=True), fork(ids_only=True), DecodePipeline(fused_vocab=True)) on the MI355X: the full-size
bf16 engine under the row-block kernel family (BOFI_RB_MIN_ROWS=0: generator + vocabulary epilogue as one rb_vocab_kernel launch), the same assertions on the
fall-back (tiled family, float32 engine), the fork without the vocabulary-wide buffers, the pipeline."""
import pytest
import torch

from conftest import load_golden, record_parity

pytestmark = pytest.mark.gpu

STAT_BAR = 2e-5          # the project's bar for the two row statistics (test_gpu_naic.py, test_entropy_perplexity_without_materialising_logprobs)
LAYOUT = ("phrase_num", "phrase_length", "phrase_syn", "bound_iters")


def _family(monkeypatch, min_rows):
    from boficap_amd import hip
    monkeypatch.setenv("BOFI_RB_MIN_ROWS", str(min_rows))
    hip.lib().bofi_reload_env()


@pytest.fixture(autouse=True)
def _restore_env(monkeypatch):
    yield
    from boficap_amd import hip
    monkeypatch.undo()
    hip.lib().bofi_reload_env()


@pytest.fixture(scope="module")
def full(weight_cache):
    """The full-size bf16 engine and 5 ragged images (region counts 50, 17, 36, 1, 44; garbage in the padding)."""
    from boficap_amd import weights as W
    from boficap_amd.engine import BofiEngine
    assert torch.cuda.is_available(), "these tests need the MI355X"
    cfg, sd = weight_cache("FULL", 0, 1.0)
    eng = BofiEngine(cfg, torch.bfloat16, max_batch=8, max_regions=50)
    eng.load_state_dict(sd)
    att_np = W.synthetic_att_feats(6, 50, cfg.att_feat_size, seed=21)
    lens = [50, 17, 36, 1, 44, 29]
    for b, n in enumerate(lens):
        att_np[b, n:] = 7.0
    att = torch.from_numpy(att_np).cuda().to(torch.bfloat16)
    return cfg, eng, att, torch.tensor(lens, dtype=torch.int32, device="cuda")


def _same(a, b, keys):
    return all(torch.equal(a[k], b[k]) for k in keys)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check_against_plain(eng, att, lens, tag, **kw):
    """The assertions of an ids-only decode against the plain decodes of the same inputs."""
    plain = eng.decode_naic(att, lens, row_stats=True, **kw)
    raw = eng.decode_naic(att, lens, raw_logits=True, **kw)
    ids = eng.decode_naic(att, lens, ids_only=True, row_stats=True, **kw)
    torch.cuda.synchronize()
    assert ids["seq_logprob"] is None
    assert _same(ids, plain, LAYOUT)
    assert torch.equal(ids["seq"], raw["seq"])                   # the greedy pick over the raw logits, bit for bit
    diff = (ids["seq"] != plain["seq"]).nonzero()
    for b, t in diff.tolist():                                   # against the log-softmax pick: only where the two ids' log-probs are one float32
        row = plain["seq_logprob"][b, t]
        assert float(row[ids["seq"][b, t]]) == float(row[plain["seq"][b, t]]), (b, t)
    for k in ("row_plogp", "row_chosen"):
        assert torch.equal(ids[k].isnan(), plain[k].isnan()), k
    e1 = float((ids["row_plogp"] - plain["row_plogp"]).nan_to_num().abs().max())
    e2 = float((ids["row_chosen"] - plain["row_chosen"]).nan_to_num().abs().max())
    print(f"ids_only {tag}: differing ids {len(diff)}, |row_plogp| diff max {e1:.3e}, |row_chosen| diff max {e2:.3e}")
    record_parity(f"ids_only_row_plogp_{tag}", e1, STAT_BAR, "decode_naic(ids_only=True) against the plain decode's row statistics, 5 ragged images")
    record_parity(f"ids_only_row_chosen_{tag}", e2, STAT_BAR, "as above, log-prob of the emitted id")
    assert e1 <= STAT_BAR and e2 <= STAT_BAR
    return ids


def test_ids_only_decode_equals_the_plain_decode(full, monkeypatch):
    cfg, eng, att6, lens6 = full
    att, lens = att6[:5], lens6[:5]
    _family(monkeypatch, 0)
    assert eng.ids_only_fused(5)
    ids = _check_against_plain(eng, att, lens, "fused")
    # eager == graph replay (captured, then replayed), bit for bit
    g = eng.decode_naic(att, lens, ids_only=True, row_stats=True, graph=True)
    g = eng.decode_naic(att, lens, ids_only=True, row_stats=True, graph=True, out=g)
    torch.cuda.synchronize()
    assert _same(g, ids, LAYOUT + ("seq",)) and torch.equal(_bits(g["row_plogp"]), _bits(ids["row_plogp"])) and torch.equal(_bits(g["row_chosen"]), _bits(ids["row_chosen"]))
    # a refinement round: every round is one fused launch; the ids are the raw-logit decode's
    _check_against_plain(eng, att, lens, "fused_refine1", refine_rounds=1)


def test_ids_only_refuses_what_it_cannot_give(full, monkeypatch):
    from boficap_amd.hip import BofiHipError
    cfg, eng, att6, lens6 = full
    _family(monkeypatch, 0)
    with pytest.raises(BofiHipError):
        eng.decode_naic(att6, lens6, ids_only=True, raw_logits=True)
    plain = eng.decode_naic(att6, lens6)
    with pytest.raises(BofiHipError):
        eng.decode_naic(att6, lens6, ids_only=True, out=plain)          # carries a seq_logprob buffer
    ids = eng.decode_naic(att6, lens6, ids_only=True)
    with pytest.raises(BofiHipError):
        eng.row_stats(ids)                                               # no distribution to read back


def test_ids_only_two_batches_in_one_launch(full, monkeypatch):
    cfg, eng, att6, lens6 = full
    _family(monkeypatch, 0)
    both = eng.decode_naic(att6, lens6, ids_only=True, row_stats=True, q1_group=3)
    torch.cuda.synchronize()
    for i in (0, 3):
        own = eng.decode_naic(att6[i:i + 3].contiguous(), lens6[i:i + 3].contiguous(), ids_only=True, row_stats=True)
        torch.cuda.synchronize()
        for k in ("seq", "phrase_num", "phrase_length", "phrase_syn"):
            assert torch.equal(both[k][i:i + 3], own[k]), (i, k)
        for k in ("row_plogp", "row_chosen"):
            assert torch.equal(_bits(both[k][i:i + 3]), _bits(own[k])), (i, k)


def test_ids_only_quirk_q1_empty_last_image(full, monkeypatch):
    """The last image without regions: under quirk Q1 every row of the batch is NaN -- all-zero ids and NaN statistics, as the plain decode gives."""
    cfg, eng, att6, lens6 = full
    _family(monkeypatch, 0)
    lens = lens6[:5].clone()
    lens[4] = 0
    plain = eng.decode_naic(att6[:5], lens, row_stats=True)
    ids = eng.decode_naic(att6[:5], lens, ids_only=True, row_stats=True)
    torch.cuda.synchronize()
    assert _same(ids, plain, LAYOUT + ("seq",))
    assert torch.equal(ids["row_plogp"].isnan(), plain["row_plogp"].isnan()) and torch.equal(ids["row_chosen"].isnan(), plain["row_chosen"].isnan())
    assert plain["row_plogp"].isnan().all() and int(ids["seq"].abs().sum()) == 0 and ids["row_plogp"].isnan().all() and ids["row_chosen"].isnan().all()


def test_ids_only_fallback_tiled_family(full, monkeypatch):
    cfg, eng, att6, lens6 = full
    _family(monkeypatch, 1 << 30)
    assert not eng.ids_only_fused(5)
    _check_against_plain(eng, att6[:5], lens6[:5], "tiled")


def test_ids_only_fallback_float32_engine(weight_cache, manifest, monkeypatch):
    from boficap_amd.engine import BofiEngine
    m = manifest["tiny_ragged"]
    cfg, sd = weight_cache(m["config"], m["seed"], m["gen_scale"], m["digest"], m.get("patch"))
    eng = BofiEngine(cfg, torch.float32, max_batch=64, max_regions=36)
    eng.load_state_dict(sd)
    g = load_golden("tiny_ragged")
    att = torch.from_numpy(g["att_feats"]).cuda()
    lens = torch.from_numpy(g["att_masks"]).sum(1).to(torch.int32).cuda()
    _family(monkeypatch, 0)
    assert not eng.ids_only_fused(att.size(0))
    _check_against_plain(eng, att, lens, "float32_tiny")


def test_ids_only_fork(full, monkeypatch):
    """A fork without the vocabulary-wide buffers: flagged decodes that take the fused generator only, and at least B * S * Npad * 4 bytes less device memory than a
    plain fork of the same size (derived: the padded generator output alone; the engine allocates with hipMalloc, so the device's free memory is what is read)."""
    from boficap_amd.hip import BofiHipError
    cfg, eng, att6, lens6 = full
    att, lens = att6[:5], lens6[:5]
    _family(monkeypatch, 0)
    B, S, Npad = 64, cfg.seq_length, -(-cfg.tgt_vocab // 128) * 128
    torch.cuda.synchronize()
    f0 = torch.cuda.mem_get_info()[0]
    plain_fork = eng.fork(max_batch=B)
    f1 = torch.cuda.mem_get_info()[0]
    fork = eng.fork(max_batch=B, ids_only=True)
    f2 = torch.cuda.mem_get_info()[0]
    print(f"fork of {B} images: plain {(f0 - f1) / 2**20:.1f} MiB, ids-only {(f1 - f2) / 2**20:.1f} MiB")
    assert (f0 - f1) - (f1 - f2) >= B * S * Npad * 4
    del plain_fork
    want = eng.decode_naic(att, lens, ids_only=True, row_stats=True)
    got = fork.decode_naic(att, lens, ids_only=True, row_stats=True)
    torch.cuda.synchronize()
    assert _same(got, want, LAYOUT + ("seq",)) and torch.equal(_bits(got["row_plogp"]), _bits(want["row_plogp"])) and torch.equal(_bits(got["row_chosen"]), _bits(want["row_chosen"]))
    with pytest.raises(BofiHipError, match="status 3"):
        fork.decode_naic(att, lens)                               # BOFI_ERR_STATE: no buffers for the distribution
    with pytest.raises(BofiHipError, match="status 3"):
        fork.decode_saic(att, lens)
    _family(monkeypatch, 1 << 30)                                 # the tiled family would need the buffers after all
    with pytest.raises(BofiHipError, match="status 3"):
        fork.decode_naic(att, lens, ids_only=True)


def test_pipeline_with_fused_vocab(full, monkeypatch):
    from boficap_amd.engine import DecodePipeline
    from boficap_amd.hip import BofiHipError
    cfg, eng, att6, lens6 = full
    _family(monkeypatch, 0)
    with pytest.raises(BofiHipError):
        DecodePipeline(eng, fused_vocab=True, keep_logprob=True)
    batches = [(att6[i:i + 2].contiguous(), lens6[i:i + 2].contiguous()) for i in (0, 2, 4)]
    pipe = DecodePipeline(eng, in_flight=2, batches_per_launch=2, fused_vocab=True, region_buckets=(50,))
    got = list(pipe.run(batches))
    assert len(got) == 3
    ref = eng.fork(max_batch=4)
    ref.set_decodes_in_flight(2)
    for (a, ln), r in zip(batches, got):
        w = ref.decode_naic(a, ln, ids_only=True, row_stats=True)
        ent, ppl = ref.entropy_perplexity(w)
        torch.cuda.synchronize()
        for k in ("seq", "phrase_num", "phrase_length", "phrase_syn"):
            assert torch.equal(r[k], w[k].cpu()), k
        assert torch.equal(_bits(r["entropy"]), _bits(ent.cpu())) and torch.equal(_bits(r["perplexity"]), _bits(ppl.cpu()))
