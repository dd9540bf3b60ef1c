"""tests/logits_rules_refs.py checked on its own (CPU only): the float64 restatement of the logits rules against the
oracle's float32 one (two texts written from SURVEY.md A.3 independently), and every input of
tests/test_gpu_logits_rules.py shown to do what it is for — an input that could not tell the right kernel from a subtly
wrong one would make the GPU test pass for nothing."""
import numpy as np
import pytest

from logits_rules_refs import (GAP, N_STATES, PLACED, SENT_F, SENT_I, family_rows, few_candidates_case, launch_ref,
                               placed_ids, placed_rows, row_histories, rule_cases, rules_ref64, rules_ref64_full, spacing32, suppress_list,
                               timestamp_state, top_gap, top_ref)

VOCABS = ["micro", "tiny.en", "large-v3"]


@pytest.fixture(scope="module", params=VOCABS)
def cfg(request):
    from faster_whisper_amd import get_config
    return get_config(request.param)


def _oracle(cfg):
    """_process_logits reads nothing but the config: no weights, no network"""
    from oracle.whisper import OracleWhisper
    o = OracleWhisper.__new__(OracleWhisper)
    o.cfg = cfg
    return o


def _oracle_lp(oracle, row, hist, with_ts, opt):
    V = row.shape[0]
    mask = None
    if opt.get("suppress_tokens"):
        mask = np.zeros(V, dtype=bool)
        mask[[t for t in opt["suppress_tokens"] if 0 <= t < V]] = True
    return oracle._process_logits(row, list(hist or []), with_ts, mask, bool(opt.get("suppress_blank", True)),
                                  int(opt.get("max_initial_timestamp_index", 50)), float(opt.get("repetition_penalty", 1.0)),
                                  int(opt.get("no_repeat_ngram_size", 0)), int(opt.get("min_new_tokens", 0)))


def _ref_lp(cfg, row, hist, with_ts, opt):
    return rules_ref64(cfg, row, list(hist or []), with_ts, opt.get("suppress_tokens"), bool(opt.get("suppress_blank", True)),
                       opt.get("max_initial_timestamp_index", 50), float(opt.get("repetition_penalty", 1.0)),
                       int(opt.get("no_repeat_ngram_size", 0)), int(opt.get("min_new_tokens", 0)))


def _inputs(cfg, family):
    """(rows [2][V], history, with_ts, options) of every kind of launch the GPU file makes on `family`"""
    tb = cfg.timestamp_begin
    out = []
    if family in ("signed", "wide"):
        for i, (_, hist, opt, spiked) in enumerate(rule_cases(cfg, np.random.default_rng(7))):
            out.append((family_rows(cfg, family, 2, 100 + i, spiked), hist, False, opt))
        for n in (4, 5):
            for r, h in enumerate(row_histories(cfg, N_STATES, n)):
                out.append((family_rows(cfg, family, 2, 200 + r), h, True,
                            dict(repetition_penalty=1.3, no_repeat_ngram_size=2)))
        for mits in (-1, 0, 3, 50, 1500, 1501, 100000, 2 ** 31 - 1):
            out.append((family_rows(cfg, family, 2, 300), None, True, dict(max_initial_timestamp_index=mits)))
    elif family == "tied":
        out.append((family_rows(cfg, "tied", 2, 400), None, False, dict(suppress_blank=False)))
        out.append((family_rows(cfg, "tied", 2, 401), [tb + 3, 40], True, dict(suppress_tokens=suppress_list(cfg))))
    else:
        rng = np.random.default_rng(500)
        out.append((placed_rows(cfg, 2, rng, False), None, False, dict(suppress_blank=False)))
        out.append((placed_rows(cfg, 2, rng, False), [11], False, dict(suppress_tokens=suppress_list(cfg))))
        out.append((placed_rows(cfg, 2, rng, True), [tb + 3, 40], True, {}))
    return out


@pytest.mark.parametrize("family", ["signed", "wide", "tied", "placed"])
def test_two_restatements_agree(cfg, family):
    """rules_ref64 (float64, from the survey) and oracle._process_logits (float32) mask the same ids and their finite
    log-probs agree to float32 round-off: one spacing for the oracle's x - max and final subtraction (half each, at the
    largest |lp|), one for its float32 log-sum-exp"""
    oracle = _oracle(cfg)
    worst, worst_sp, lp_max = 0.0, 0.0, 0.0
    for rows, hist, with_ts, opt in _inputs(cfg, family):
        for row in rows:
            got32, lp = _ref_lp(cfg, row, hist, with_ts, opt)
            ref = _oracle_lp(oracle, row, hist, with_ts, opt)
            fin = np.isfinite(lp)
            assert np.array_equal(fin, np.isfinite(ref)), (family, hist, opt)
            if not fin.any():
                continue
            d = np.abs(lp[fin] - ref[fin].astype(np.float64))
            sp = spacing32(np.abs(lp[fin]).max())
            worst, worst_sp, lp_max = max(worst, d.max()), max(worst_sp, d.max() / sp), max(lp_max, np.abs(lp[fin]).max())
            assert d.max() <= 2.0 * sp, (family, hist, opt, d.max(), sp)
    print(f"[{cfg.name}] {family}: worst |ref64 - oracle32| = {worst:.2e} ({worst_sp:.2f} float32 spacings) at max |lp| = {lp_max:.0f}")
    # the ranges the value bounds of the GPU test rest on: the project's range (2e-5 absolute is 10.5 spacings below 32;
    # the tied and placed rows reach a little further) and, wide, the binade of 261 = 128 + 128 + ln V (a penalised
    # -128 * 1.3 stays inside it): a condition on the inputs, not on the kernel
    assert lp_max < {"signed": 32.0, "wide": 512.0}.get(family, 64.0)


def test_signed_penalty_acts_on_both_sides_of_zero(cfg):
    """... and a kernel that divides negative values too is told apart, in the row and in the candidates"""
    name, hist, opt, spiked = rule_cases(cfg, np.random.default_rng(7))[3]
    assert name == "penalty 1.3"
    lg = family_rows(cfg, "signed", 2, 103, spiked)
    ids = sorted(set(hist))
    assert (lg[:, ids] < 0).any(axis=1).all() and (lg[:, ids] > 0).any(axis=1).all()
    print(f"[{cfg.name}] penalised ids {ids}: row 0 holds {lg[0, ids]}")
    cum = np.zeros(2, np.float32)
    for K in (1, 5, 16):
        good = launch_ref(cfg, lg, [hist] * 2, cum, K, False, **opt)
        bad = launch_ref(cfg, lg, [hist] * 2, cum, K, False, defect="negdiv", **opt)
        assert not np.array_equal(good["logits"], bad["logits"])
        ch = good["logits"] != bad["logits"]
        assert ch.any(axis=1).all() and (good["logits"][ch] < bad["logits"][ch]).all() and (lg[ch] < 0).all()
    # with the whole row below zero the penalised ids ARE the best ones: the candidates differ too
    name, hist_n, opt_n, spiked_n = rule_cases(cfg, np.random.default_rng(7))[5]
    assert "all-negative" in name
    neg = family_rows(cfg, "signed", 2, 105, spiked_n)
    assert neg.max() < 0 and (neg[:, 20] == neg.max(axis=1)).all()
    for K in (1, 5, 16):
        good = launch_ref(cfg, neg, [hist_n] * 2, cum, K, False, **opt_n)
        bad = launch_ref(cfg, neg, [hist_n] * 2, cum, K, False, defect="negdiv", **opt_n)
        assert (bad["tok"][:, 0] == 20).all() and (good["tok"][:, :2 * K] != 20).all()
    # 0.8 lifts the spiked ids to the top: the order of the candidates changes with the penalty
    opt8 = rule_cases(cfg, np.random.default_rng(7))[4][2]
    plain = launch_ref(cfg, lg, [hist] * 2, cum, 5, False)
    pen = launch_ref(cfg, lg, [hist] * 2, cum, 5, False, **opt8)
    assert (pen["tok"][:, 0] == 20).all() and (pen["tok"][:, 1] == 0).all() and (plain["tok"][:, 0] == 20).all()
    assert not np.array_equal(plain["val"], pen["val"])


def test_tied_inputs_and_tie_break_defects(cfg):
    V = cfg.n_vocab
    lg = family_rows(cfg, "tied", 2, 400)
    n_top = int((lg[0] == lg[0].max()).sum())
    print(f"[{cfg.name}] tied family: {n_top} ids at the top level of row 0 (V = {V})")
    if V > 4096:
        assert n_top > 32                                           # more tied ids at the top value than 2K, K = 16
    cum = np.array([-0.5, -1.25], np.float32)
    # identical raw values give identical log-probs: "id for id" is well defined under ties
    _, lp = _ref_lp(cfg, lg[0], None, False, dict(suppress_blank=False))
    for level in np.unique(lg[0])[-3:]:
        assert np.unique(lp[lg[0] == level]).size == 1
    for K in (1, 5, 16):
        good = launch_ref(cfg, lg, None, cum, K, False, suppress_blank=False)
        for d in ("highest", "thread"):
            bad = launch_ref(cfg, lg, None, cum, K, False, suppress_blank=False, defect=d)
            if d == "highest" or V > 4096 or K == 16:               # (micro, "thread": its 30 top ids need 2K = 32 slots)
                assert not np.array_equal(good["tok"], bad["tok"]), (K, d)
    # placed ties: ascending ids, then the next level; each wrong order changes the expected ids
    for text_only, hist, with_ts, opt in ((False, None, False, dict(suppress_blank=False)),
                                          (False, [11], False, dict(suppress_tokens=suppress_list(cfg))),
                                          (True, [cfg.timestamp_begin + 3, 40], True, {})):
        pl = placed_rows(cfg, 2, np.random.default_rng(500), text_only)
        ids = placed_ids(cfg, text_only)
        assert len(ids) >= 6 and (pl[:, ids] == PLACED).all() and (pl == PLACED).sum() == 2 * len(ids)
        left = [t for t in ids if t not in (opt.get("suppress_tokens") or [])]
        assert 2 <= len(left) and (len(left) < len(ids)) == bool(opt.get("suppress_tokens"))
        hs = None if hist is None else [hist] * 2
        good = launch_ref(cfg, pl, hs, cum, 16, with_ts, **opt)
        assert with_ts is False or good["margins"][0] < -1.0        # the text ids survive rule (e)
        assert good["tok"][0, :len(left)].tolist() == left          # ascending ids
        nxt = good["val"][0, len(left):32]
        assert (nxt < good["val"][0, 0] - 1.0).all() and np.unique(nxt).size == 1 and np.isfinite(nxt).all()
        assert (np.diff(good["tok"][0, len(left):32]) > 0).all()    # ... then the next level, ascending again
        for d in ("highest", "thread"):
            bad = launch_ref(cfg, pl, hs, cum, 16, with_ts, defect=d, **opt)
            assert not np.array_equal(good["tok"][:, :len(left)], bad["tok"][:, :len(left)]) or \
                (d == "thread" and max(left) < 1024), (d, left)
            assert not np.array_equal(good["tok"], bad["tok"]), d


@pytest.mark.parametrize("family", ["signed", "wide"])
def test_distinct_families_decide_the_order(cfg, family):
    """the smallest gap among the best 2K + 1 values of every row of every distinct-family launch is at least GAP: far
    above any round-off, so the candidate ids are decided"""
    worst = float("inf")
    for rows, hist, with_ts, opt in _inputs(cfg, family):
        for row in rows:
            _, lp = _ref_lp(cfg, row, hist, with_ts, opt)
            worst = min(worst, top_gap(lp, 16))
    print(f"[{cfg.name}] {family}: smallest gap among the best 33 values of a row = {worst:.3e}")
    assert worst >= GAP


def test_per_row_histories_differ_and_row0_defect_shows(cfg):
    tb = cfg.timestamp_begin
    for n in (4, 5):
        hs = row_histories(cfg, 15, n)
        # (a closed pair and text after the last timestamp id forbid the same ids by different routes: the third entry)
        states = [timestamp_state(cfg, h) + (h[-1] >= tb,) for h in hs[:N_STATES]]
        print(f"[{cfg.name}] n = {n}: (a_hi, b_hi, last token a timestamp) of the five states = {states}")
        assert len(set(states)) == N_STATES
        assert states[2][1] == cfg.n_vocab and states[4][1] == cfg.n_vocab and states[3][:2] == (cfg.eot, cfg.n_vocab - 1)
        assert all(len(h) == n for h in hs) and len({tuple(h) for h in hs}) == len(hs)
        lg = family_rows(cfg, "signed", 15, 600 + n)
        cum = -np.arange(15, dtype=np.float32) / 8
        opt = dict(repetition_penalty=1.3, no_repeat_ngram_size=2)
        good = launch_ref(cfg, lg, hs, cum, 5, True, **opt)
        bad = launch_ref(cfg, lg, hs, cum, 5, True, defect="row0", **opt)
        for r in range(1, 15):
            assert not np.array_equal(good["tok"][r], bad["tok"][r]) or not np.array_equal(good["logits"][r], bad["logits"][r]), r
        assert sum(not np.array_equal(good["tok"][r], bad["tok"][r]) for r in range(1, 15)) >= 8
        # rule (e) is decided in every row where both classes are alive
        m = np.array(good["margins"])
        assert (np.abs(m[np.isfinite(m)]) >= GAP).all(), m
        # the last-timestamp states leave what they should
        assert set(good["tok"][3, :10][np.isfinite(good["val"][3, :10])]) <= {cfg.n_vocab - 1} | set(range(cfg.eot, tb))
        assert (good["tok"][4, :10][np.isfinite(good["val"][4, :10])] < tb).all()


def test_done_defect_shows(cfg):
    lg = family_rows(cfg, "signed", 6, 700)
    hs = row_histories(cfg, 6, 4)
    cum = np.zeros(6, np.float32)
    opt = dict(repetition_penalty=1.3)
    for done in ([0, 1, 0], [1, 0, 1]):
        good = launch_ref(cfg, lg, hs, cum, 2, True, done=done, **opt)
        bad = launch_ref(cfg, lg, hs, cum, 2, True, done=done, defect="done", **opt)
        for c in range(3):
            rows = slice(2 * c, 2 * c + 2)
            if done[c]:
                assert (good["tok"][rows] == SENT_I).all() and (good["val"][rows] == SENT_F).all()
                assert np.array_equal(good["logits"][rows], lg[rows])
                assert (bad["tok"][rows, :4] != SENT_I).all() and not np.array_equal(bad["logits"][rows], lg[rows])
            else:
                assert np.array_equal(good["tok"][rows], bad["tok"][rows])
                assert (good["tok"][rows, 4:] == SENT_I).all() and (good["tok"][rows, :4] != SENT_I).all()


def test_first_step_limits_and_few_candidates(cfg):
    """mits 0 / 3 leave 1 / 4 live candidates, every value from the number of timestamp ids on leaves them all; the
    few-candidates case leaves exactly 4"""
    tb, V = cfg.timestamp_begin, cfg.n_vocab
    lg = family_rows(cfg, "signed", 1, 300)
    cum = np.zeros(1, np.float32)
    free = launch_ref(cfg, lg, None, cum, 16, True, max_initial_timestamp_index=-1)
    assert np.isfinite(free["val"][0, :32]).all() and (free["tok"][0, :32] >= tb).all()
    for mits, live in ((0, 1), (3, 4), (50, 32), (1500, 32), (1501, 32), (100000, 32), (2 ** 31 - 1, 32)):
        got = launch_ref(cfg, lg, None, cum, 16, True, max_initial_timestamp_index=mits)
        assert int(np.isfinite(got["val"][0, :32]).sum()) == live
        assert (got["tok"][0, live:32] == 0).all() and (got["tok"][0, :live] <= tb + mits).all()
        if mits >= 1500:
            assert np.array_equal(got["tok"], free["tok"]) and np.array_equal(got["val"], free["val"])
    hist, opt, keep = few_candidates_case(cfg)
    got = launch_ref(cfg, lg, [hist], cum, 16, True, **opt)
    assert int(np.isfinite(got["val"][0, :32]).sum()) == 4 and set(got["tok"][0, :4]) == set(keep)


def test_spacing32():
    x = np.array([1.0, 1.5, 2.0, 31.9, 32.0, 261.0, 0.0, 1e-45], np.float64)
    want = [np.spacing(np.float32(v)) for v in x[:6]] + [2.0 ** -149, 2.0 ** -149]
    assert spacing32(x).tolist() == [float(w) for w in want]
    assert 2e-5 / spacing32(31.0) == pytest.approx(10.5, abs=0.02)   # the value bound of the GPU tests, in spacings
