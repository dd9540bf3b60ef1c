"""The references of the scoring tests (tests/score_refs.py), on the CPU:

  * its rule-mode restatement (the oracle's _process_logits decides which ids are forbidden) equals the float64
    restatement written from the survey (tests/logits_rules_refs.py) on every rule-mode input of the kernel tests;
  * on those inputs rule (e) is never a tie: every margin is nan or at least score_refs.MARGIN in magnitude, for every
    seed and vocabulary the GPU tests use — so they exclude no row;
  * the inputs hold what the GPU tests say they hold (target edges, ties, -inf rows, both sides of rule (e));
  * the model-level reference (one decoder_full pass + the row reference) along the oracle's own greedy ids reproduces
    the oracle's cumulative score, and best - token equals the oracle's forced_gaps."""
import numpy as np
import pytest

import logits_rules_refs as lr
import score_refs as sr


def _cfg(name):
    """the vocabulary and token ids of `name` (what the kernel tests' models carry)"""
    from faster_whisper_amd import get_config
    return get_config(name)


@pytest.mark.parametrize("name", ["micro", "tiny", "large-v3"])
def test_rule_cases_two_restatements_agree_and_rule_e_is_never_a_tie(name):
    cfg = _cfg(name)
    sides = set()
    for seed in sr.SEEDS:
        for what, lg, t, hists, opt, with_ts in sr.rule_cases(cfg, seed):
            assert all(len(h) < cfg.n_text_ctx for h in hists), what
            ref = sr.score_rows_ref(cfg, lg, t, hists, opt, with_ts)
            m = np.array(ref["margins"])
            assert (np.abs(m[np.isfinite(m)]) >= sr.MARGIN).all(), (name, seed, what, m)
            sides |= {bool(x > 0) for x in m[np.isfinite(m)]}
            for r in range(lg.shape[0]):
                if t[r] < 0:
                    assert ref["lp"][r] == float(sr.SENT_F) and ref["best_id"][r] == sr.SENT_I
                    continue
                _, lp, _ = lr.rules_ref64_full(cfg, lg[r], hists[r], with_ts, opt.get("suppress_tokens"),
                                               opt.get("suppress_blank", True), opt.get("max_initial_timestamp_index", 50),
                                               opt.get("repetition_penalty", 1.0), opt.get("no_repeat_ngram_size", 0))
                a, b, c = sr.pick(lp, int(t[r]))
                assert b == ref["best_id"][r], (what, r)
                for x, y in ((a, ref["lp"][r]), (c, ref["best_lp"][r])):
                    assert (x == y) if not np.isfinite(y) else abs(x - y) < 1e-12, (what, r, x, y)
    assert sides == {True, False}        # rule (e) is taken on both sides
    # the longest history reaches the last position the text context has
    assert max(len(h) for _, _, _, hists, _, _ in sr.rule_cases(cfg, sr.SEEDS[0]) for h in hists) == cfg.n_text_ctx - 1


@pytest.mark.parametrize("name", ["micro", "large-v3"])
def test_rule_cases_hold_masked_and_unmasked_targets(name):
    cfg = _cfg(name)
    dead = alive = 0
    for what, lg, t, hists, opt, with_ts in sr.rule_cases(cfg, sr.SEEDS[0]):
        ref = sr.score_rows_ref(cfg, lg, t, hists, opt, with_ts)
        scored = ref["lp"][t >= 0]
        dead += int(np.isneginf(scored).sum())
        alive += int(np.isfinite(scored).sum())
        assert not np.isnan(scored).any(), what
    assert dead >= 3 and alive >= 10


def test_raw_cases_hold_their_edges():
    cfg = _cfg("micro")
    V = cfg.n_vocab
    assert V % 1024 != 0
    cases = dict((w, (lg, t)) for w, lg, t in sr.raw_cases(cfg, sr.SEEDS[0]))
    lg, t = cases["signed rows x 37"]
    assert {0, V - 1, cfg.timestamp_begin} <= set(t.tolist()) and (t < 0).sum() >= 2 and lg.shape == (37, V)
    assert cases["signed rows x 1"][0].shape == (1, V)
    lg, t = cases["-inf rows"]
    ref = sr.score_rows_ref(cfg, lg, t)
    assert ref["lp"][0] == 0.0 and ref["best_id"][0] == t[0]               # -inf everywhere but the target
    assert np.isneginf(ref["lp"][1]) and np.isfinite(ref["best_lp"][1])    # a target at -inf: -inf, not nan
    lg, t = cases["tied maxima"]
    ref = sr.score_rows_ref(cfg, lg, t)
    assert ref["best_id"].tolist() == [5, 1023, 63, V - 2] and (ref["best_id"] != t).all()
    assert np.array_equal(ref["lp"], ref["best_lp"])                        # the target is one of the tied maxima
    # magnitude 1e4: x - (M + L) in float32 loses what (x - M) - L keeps
    lg, t = cases["magnitude 1e4"]
    ref = sr.score_rows_ref(cfg, lg, t)
    M = lg.max(axis=1).astype(np.float32)
    L = np.log(np.exp((lg - M[:, None]).astype(np.float64)).sum(axis=1)).astype(np.float32)
    x = lg[np.arange(3), t]
    one_part = (x - (M + L)).astype(np.float64)
    two_part = ((x - M) - L).astype(np.float64)
    assert np.abs(two_part - ref["lp"]).max() < 2e-6 < 1e-4 < np.abs(one_part - ref["lp"]).max()


@pytest.mark.parametrize("timestamps", [False, True])
def test_model_reference_reproduces_the_oracles_greedy_score(timestamps):
    """fp32 oracle, micro geometry.  The oracle's greedy path runs position by position, the reference in one
    decoder_full pass: 1e-6 per token between the two (tests/test_oracle_decode.py); the oracle's log-softmax is
    float32 over V values, the reference's float64: < 4e-6 per token at |log-prob| < 16.  Bound: 1e-5 per token."""
    from faster_whisper_amd import get_config, synthetic_weights
    from oracle.whisper import OracleWhisper, max_new_tokens
    from conftest import forced_result
    cfg = get_config("micro")
    o = OracleWhisper(cfg, synthetic_weights(cfg, seed=3), emulate_fp16=False)
    enc = (np.random.default_rng(0).standard_normal((1500, cfg.d_model)) * 0.5).astype(np.float32)
    prompt = list(cfg.sot_sequence) + ([] if timestamps else [cfg.no_timestamps])
    rules = dict(suppress_blank=True, max_initial_timestamp_index=50, repetition_penalty=1.2, no_repeat_ngram_size=3,
                 suppress_tokens=[cfg.sot, cfg.no_speech, 1, 2, 7])
    kw = dict(rules, max_length=len(prompt) + 20, length_penalty=0.0)
    g = o.generate(enc[None], [prompt], beam_size=1, **kw)[0]
    ids = g.sequences_ids[0]
    budget = max_new_tokens(kw["max_length"], len(prompt))
    assert len(ids) >= 4
    ref = sr.model_ref(o, enc, prompt, ids, rules)
    closed = len(ids) < budget                                   # ended with <eot>: its term belongs to the score
    terms = list(ref["token_lp"]) + ([ref["end_lp"]] if closed else [])
    n = len(terms)
    cum = sr.cum32(terms)
    print(f"timestamps={timestamps}: {len(ids)} ids, closed={closed}, reference cum {cum:.6f}, oracle {g.scores[0]:.6f}")
    assert abs(cum - g.scores[0]) < 1e-5 * n, (cum, g.scores)
    assert ref["best_ids"][:len(ids)] == ids                     # a greedy sequence is its own arg-max path
    fr = forced_result(o, enc, prompt, ids, dict(kw, beam_size=1))
    gaps = (ref["best_lp"] - np.append(ref["token_lp"], ref["end_lp"]))[:len(fr.forced_gaps)]
    assert len(fr.forced_gaps) == n and np.abs(gaps - np.array(fr.forced_gaps)).max() < 1e-5
    # a sequence the search did NOT choose: the gaps are no longer zero, and still the oracle's
    other = list(ids[:3]) + [ids[3] + 1 if ids[3] + 1 < cfg.eot else ids[3] - 1] + list(ids[4:8])
    fr = forced_result(o, enc, prompt, other, dict(kw, beam_size=1))
    if np.isfinite(fr.scores[0]):
        ref = sr.model_ref(o, enc, prompt, other, rules)
        gaps = (ref["best_lp"] - np.append(ref["token_lp"], ref["end_lp"]))[:len(fr.forced_gaps)]
        assert max(fr.forced_gaps) > 0 and np.abs(gaps - np.array(fr.forced_gaps)).max() < 1e-5
        assert abs(sr.cum32(list(ref["token_lp"]) + [ref["end_lp"]]) - fr.scores[0]) < 1e-5 * (len(other) + 1)
