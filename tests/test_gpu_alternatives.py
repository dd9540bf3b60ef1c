"""generate(..., return_alternatives=N) end to end on the GPU, on the setup of tests/test_gpu_token_logprobs.py (the micro
model of seed 11, three chunks, one of them short, that file's prompt and suppress list, 12 new tokens; that file records
that no step of this setup is rule-tied).  Modes: greedy, beam 5 with 3 hypotheses, sampling with 3 hypotheses.

  1. nothing else moves: ids, scores, no-speech values, token and end log-probs are those of return_token_logprobs alone;
  2. the exact identities between the chosen tokens and the alternatives of their positions, the end slot included;
  3. against Whisper.score: scoring ids[:t] + [alternative id] with the call's rules returns the alternative's log-prob bit
     for bit (greedy), and score's best id at that position is alternative 0;
  4. against the CPU oracle (fp16-emulating and fp32), teacher-forced along the engine's own ids;
  5. calls with different N, without alternatives and with a longer prompt share decode runs, each getting its solo result;
  6. N outside [0, 8] is a ValueError.

Measured on an MI355X (test 4, micro; the larger of the two errors over the 12 positions x 8 ranks of a hypothesis, the chunk
closest to its bound per mode; band = max |oracle fp16 - oracle fp32| on the same entries, bound = max(1e-3, 3 * band); no
step was tied):
  greedy   2.069e-03 (band 1.481e-03, bound 4.443e-03)
  beam 5   2.475e-03 (band 1.504e-03, bound 4.513e-03)
  sampling 1.917e-03 (band 1.642e-03, bound 4.927e-03)
The closest case to its bound is beam 5, chunk 1: 0.55 of it.  Test 5: the four beam calls met in ONE decode run, the two
sampling calls in one."""
import threading
import time

import numpy as np
import pytest

from alternatives_refs import check_alternatives
from conftest import bench_audio, make_model

pytestmark = pytest.mark.gpu

NEW = 12
RULE_TIE = 2e-2
MODES = {
    "greedy": dict(beam_size=1),
    "beam5": dict(beam_size=5, num_hypotheses=3, patience=1.0),
    "sampling": dict(beam_size=1, num_hypotheses=3, sampling_topk=0, sampling_temperature=0.8, seed=1234),
}


@pytest.fixture(scope="module")
def setup():
    from faster_whisper_amd.backend import StorageView
    cfg, w, model = make_model("micro", seed=11, max_batch=4, max_beam=5)
    chunks = [bench_audio(480000, seed=1), bench_audio(200000, seed=2), bench_audio(480000, seed=3)[::-1].copy()]
    enc = model.encode(StorageView.from_array(model.log_mel(chunks)))
    return cfg, w, model, enc


def _prompt(cfg, timestamps=False):
    p = list(cfg.sot_sequence)
    if not timestamps:
        p.append(cfg.no_timestamps)
    return p


def _suppress(cfg):
    return sorted({cfg.sot, cfg.sot_prev, cfg.sot_lm, cfg.no_speech, cfg.translate, cfg.transcribe, 1, 2, 7})


def _kw(cfg, mode, new=NEW, timestamps=False):
    return dict(MODES[mode], max_length=len(_prompt(cfg, timestamps)) + new, suppress_tokens=_suppress(cfg),
                length_penalty=0.0, return_scores=True, return_no_speech_prob=True)


def _same(a, b, alternatives=False):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.sequences_ids == y.sequences_ids and x.scores == y.scores and x.no_speech_prob == y.no_speech_prob
        assert x.token_logprobs == y.token_logprobs and x.end_logprobs == y.end_logprobs
        if alternatives:
            assert x.token_alternatives == y.token_alternatives and x.end_alternatives == y.end_alternatives


def _check_result(cfg, res, n_alt, greedy, budget):
    """identities (2) on every hypothesis of a result list; returns (closed by <eot>, cut at the budget)"""
    closed = cut = 0
    for r in res:
        assert len(r.token_alternatives) == len(r.sequences_ids) == len(r.end_alternatives)
        for ids, lps, end, alts, end_alt in zip(r.sequences_ids, r.token_logprobs, r.end_logprobs, r.token_alternatives,
                                                r.end_alternatives):
            assert all(len(a) == n_alt for a in alts)
            check_alternatives(ids, lps, alts, greedy)
            if len(ids) == budget:                        # cut at the budget: no closing step
                assert end_alt is None and end == 0.0
                cut += 1
            else:
                assert end_alt is not None and len(end_alt) == n_alt
                check_alternatives([cfg.eot], [end], [end_alt], greedy)
                closed += 1
    return closed, cut


@pytest.mark.parametrize("timestamps", [False, True])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_outputs_unchanged_and_identities(setup, mode, timestamps):
    cfg, _, model, enc = setup
    prompt = _prompt(cfg, timestamps)
    kw = _kw(cfg, mode, timestamps=timestamps)
    base = model.generate(enc, [prompt] * 3, return_token_logprobs=True, **kw)
    assert all(r.token_alternatives == [] and r.end_alternatives == [] for r in base)
    top8 = None
    for n_alt in (8, 4, 1):
        res = model.generate(enc, [prompt] * 3, return_alternatives=n_alt, **kw)
        _same(res, base)
        _check_result(cfg, res, n_alt, mode == "greedy", NEW)
        if top8 is None:
            top8 = res
        for r, r8 in zip(res, top8):                     # the first n of the top 8 are the top n
            assert r.token_alternatives == [[a[:n_alt] for a in alts] for alts in r8.token_alternatives]
            assert r.end_alternatives == [None if a is None else a[:n_alt] for a in r8.end_alternatives]


@pytest.mark.parametrize("mode", sorted(MODES))
def test_budget_cuts_have_no_end_alternatives(setup, mode):
    """a budget of 4: some hypotheses are cut (end_alternatives None), and every id but {eot, 20, 21, 22} suppressed in a
    second call makes others close on <eot> early, some with fewer than N live ids ((0, -inf) tails)"""
    cfg, _, model, enc = setup
    prompt = _prompt(cfg)
    res = model.generate(enc, [prompt] * 3, return_alternatives=3, **_kw(cfg, mode, new=4))
    closed, cut = _check_result(cfg, res, 3, mode == "greedy", 4)
    assert cut > 0
    keep = {cfg.eot, 20, 21, 22}
    kw = dict(_kw(cfg, mode, new=4), suppress_blank=False, suppress_tokens=[t for t in range(cfg.n_vocab) if t not in keep])
    if mode == "beam5":
        kw.update(beam_size=4)
    res = model.generate(enc, [prompt] * 3, return_alternatives=8, **kw)
    closed2, cut2 = _check_result(cfg, res, 8, mode == "greedy", 4)
    print(f"[{mode}] budget 4: {closed} closed / {cut} cut; four live ids: {closed2} closed / {cut2} cut")
    for r in res:
        for alts in r.token_alternatives:
            for a in alts:
                assert {i for i, v in a if v != -np.inf} <= keep and a[4:] == [(0, -np.inf)] * 4
    if mode == "beam5":
        assert closed2 > 0 and cut2 > 0


def test_alternatives_against_score(setup):
    """greedy, every chunk, three positions (the first, the middle, the last): fw_score with the call's rules on
    ids[:t] + [alternative id] returns the alternative's log-prob bit for bit, and its best id there is alternative 0"""
    cfg, _, model, enc = setup
    prompt = _prompt(cfg, True)
    kw = dict(_kw(cfg, "greedy", timestamps=True), repetition_penalty=1.2, no_repeat_ngram_size=3)
    rules = dict(suppress_tokens=kw["suppress_tokens"], repetition_penalty=1.2, no_repeat_ngram_size=3)
    res = model.generate(enc, [prompt] * 3, return_alternatives=5, **kw)
    _check_result(cfg, res, 5, True, NEW)
    n = min(len(r.sequences_ids[0]) for r in res)
    assert n >= 3
    for t in (0, n // 2, n - 1):
        targets = [[r.sequences_ids[0][:t] + [alt_id] for alt_id, _ in r.token_alternatives[0][t]] for r in res]
        sc = model.score(enc, [prompt] * 3, targets, rules=True, **rules)
        for r, s in zip(res, sc):
            alts = r.token_alternatives[0][t]
            for h, (alt_id, alt_lp) in enumerate(alts):
                got = s.token_logprobs[h][t]
                assert np.float32(got).view(np.uint32) == np.float32(alt_lp).view(np.uint32), (t, h, alt_id, got, alt_lp)
                assert s.best_ids[h][t] == alts[0][0]


# ------------------------------------------------------------------------------------------------ against the oracle
def _oracle_top(oracle, enc_b, prompt, ids, sup, n):
    """the oracle teacher-forced along ids in ONE pass: per position 0 .. len(ids) (the last is the closing step) the
    processed log-probs [V]; returns (rows [len + 1][V], rule margins)"""
    import torch
    from oracle.whisper import _t
    P = len(prompt)
    with_ts = oracle.cfg.no_timestamps not in prompt
    with torch.no_grad():
        ckv = oracle.cross_kv(oracle._r(_t(enc_b[None])))
        hid = oracle.decoder_full(torch.tensor([list(prompt) + list(ids)], dtype=torch.long), ckv)
        lg = oracle.logits(hid[0, P - 1:P + len(ids)]).numpy()
    rows, margins = [], []
    for t in range(len(ids) + 1):
        rows.append(oracle._process_logits(lg[t], list(ids[:t]), with_ts, sup, True, 50, 1.0, 0, 0))
        margins.append(oracle._rule_margin)
    return np.stack(rows), margins


@pytest.fixture(scope="module")
def oracles(setup):
    from oracle.whisper import OracleWhisper
    cfg, w, model, enc = setup
    return enc.to_numpy(), OracleWhisper(cfg, w, emulate_fp16=True), OracleWhisper(cfg, w, emulate_fp16=False)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_alternatives_against_the_oracle(setup, oracles, mode):
    """rank by rank |engine lp_j - oracle16 lp_j| and by id |oracle16 lp[engine id_j] - oracle16 lp_j|, both
    <= max(1e-3, 3 * band), band = max |oracle16 - oracle32| over the same entries (the bound of
    tests/test_gpu_token_logprobs.py, for its reason).  No id equality is demanded: near-ties need no exemption.  Steps where
    timestamp rule (e) is tied (|rule margin| < 2e-2) are printed and left out, at most one per hypothesis."""
    cfg, _, model, enc = setup
    enc_np, o16, o32 = oracles
    prompt = _prompt(cfg)
    N = 8
    res = model.generate(enc, [prompt] * 3, return_alternatives=N, **_kw(cfg, mode))
    sup = np.asarray(_suppress(cfg), dtype=np.int64)
    for b, r in enumerate(res):
        ids = r.sequences_ids[0]
        alts = list(r.token_alternatives[0]) + ([r.end_alternatives[0]] if r.end_alternatives[0] is not None else [])
        assert 1 <= len(alts) <= NEW + 1
        lp16, margins = _oracle_top(o16, enc_np[b], prompt, ids, sup, N)
        lp32, _ = _oracle_top(o32, enc_np[b], prompt, ids, sup, N)
        tied = [t for t, m in enumerate(margins[:len(alts)]) if m == m and abs(m) < RULE_TIE]
        if tied:
            print(f"[{mode}] chunk {b}: rule (e) tied at step(s) {tied}: left out")
        assert len(tied) <= 1
        err = band = 0.0
        for t, alt in enumerate(alts):
            if t in tied:
                continue
            s16, s32 = -np.sort(-lp16[t].astype(np.float64))[:N], -np.sort(-lp32[t].astype(np.float64))[:N]
            e_ids = np.asarray([i for i, _ in alt])
            e_lp = np.asarray([v for _, v in alt], np.float64)
            assert np.isfinite(e_lp).all() and np.isfinite(s16).all()
            by_id16, by_id32 = lp16[t][e_ids].astype(np.float64), lp32[t][e_ids].astype(np.float64)
            err = max(err, float(np.abs(e_lp - s16).max()), float(np.abs(by_id16 - s16).max()))
            band = max(band, float(np.abs(s16 - s32).max()), float(np.abs(by_id16 - by_id32).max()))
        bound = max(1e-3, 3 * band)
        print(f"[{mode}] chunk {b}: {len(alts)} positions x {N} ranks: max error {err:.3e}, band {band:.3e}, bound {bound:.3e}")
        assert err <= bound, (mode, b, err, bound)


# ------------------------------------------------------------------------------------------------------- shared runs
def _group_model():
    from faster_whisper_amd import Whisper, get_config, synthetic_weights
    cfg = get_config("micro")
    model = Whisper("synthetic:micro", device="cuda", files={"config": cfg, "weights": synthetic_weights(cfg, seed=21)},
                    max_batch_size=3, max_beam_size=5, inter_threads=4)
    model.set_decode_lanes(1)            # one run at a time: what is queued behind the blocker meets in the next one
    return cfg, model


def _behind_a_blocker(model, cfg, batches, prompts, kws):
    """the calls are queued from one thread each while a run they cannot share (beam 2, <eot> suppressed, the whole text
    context) holds the only lane; returns (results, decode runs the calls took)"""
    n = len(batches)
    out, errs = [None] * n, []
    encoded, go = threading.Barrier(n + 1), threading.Event()

    def work(i):
        try:
            e = model.encode_pcm(batches[i])
            encoded.wait(timeout=120)
            assert go.wait(timeout=120)
            out[i] = model.generate(e, [prompts[i]] * len(batches[i]), **kws[i])
        except Exception as ex:   # noqa: BLE001
            errs.append(ex)

    blocker_enc = model.encode_pcm(batches[0])
    ts = [threading.Thread(target=work, args=(i,)) for i in range(n)]
    for t in ts:
        t.start()
    encoded.wait(timeout=120)
    st0 = model.decode_stats()
    tb = threading.Thread(target=lambda: model.generate(blocker_enc, [prompts[0]] * len(batches[0]), beam_size=2,
                                                        max_length=cfg.n_text_ctx, suppress_tokens=[cfg.eot]))
    tb.start()
    t_end = time.time() + 30
    while model.decode_stats()["runs"] == st0["runs"] and time.time() < t_end:
        pass                                   # until the blocker's run has started
    go.set()
    for t in ts + [tb]:
        t.join()
    assert not errs, errs
    st = model.decode_stats()
    assert st["requests"] - st0["requests"] == n + 1
    return out, st["runs"] - st0["runs"] - 1


def _batches(sizes):
    return [[bench_audio(480000 if (i + j) % 3 else 250000, seed=50 + 10 * i + j) for j in range(n)]
            for i, n in enumerate(sizes)]


def test_calls_of_different_n_share_runs():
    """four beam-5 calls — without alternatives, with 3, with 8, and with 3 behind a longer prompt (a ragged run) — meet in
    fewer runs than calls; every call's full result is its solo result, bit for bit"""
    cfg, model = _group_model()
    short = _prompt(cfg)
    longer = [cfg.sot_prev] + [10 + (7 * i) % 200 for i in range(17)] + short
    prompts = [short, short, short, longer]
    base = dict(beam_size=5, num_hypotheses=3, max_length=len(longer) + 10, length_penalty=0.0, return_scores=True,
                return_no_speech_prob=True, suppress_tokens=[cfg.sot, cfg.no_speech, 1, 2])
    kws = [dict(base, return_token_logprobs=True), dict(base, return_alternatives=3), dict(base, return_alternatives=8),
           dict(base, return_alternatives=3)]
    batches = _batches((3, 2, 3, 2))
    solo = [model.generate(model.encode_pcm(b), [p] * len(b), **kw) for b, p, kw in zip(batches, prompts, kws)]
    for s, n_alt, p in zip(solo[1:], (3, 8, 3), prompts[1:]):
        _check_result(cfg, s, n_alt, False, base["max_length"] - len(p))
    out, runs = _behind_a_blocker(model, cfg, batches, prompts, kws)
    print(f"4 calls (N = 0, 3, 8, 3 ragged) -> {runs} decode run(s)")
    assert runs < 4
    for o, s in zip(out, solo):
        _same(o, s, alternatives=True)
    assert all(r.token_alternatives == [] for r in out[0])
    assert all(len(a) == 8 for r in out[2] for alts in r.token_alternatives for a in alts)


def test_sampling_calls_of_different_n_share_a_run():
    cfg, model = _group_model()
    prompt = _prompt(cfg)
    base = dict(beam_size=1, num_hypotheses=3, sampling_topk=0, max_length=len(prompt) + 10, length_penalty=0.0,
                return_scores=True, return_no_speech_prob=True, suppress_tokens=[cfg.sot, cfg.no_speech, 1, 2])
    kws = [dict(base, sampling_temperature=0.6, seed=7, return_alternatives=2),
           dict(base, sampling_temperature=1.0, seed=11, return_alternatives=8)]
    batches = _batches((2, 3))
    solo = [model.generate(model.encode_pcm(b), [prompt] * len(b), **kw) for b, kw in zip(batches, kws)]
    out, runs = _behind_a_blocker(model, cfg, batches, [prompt] * 2, kws)
    print(f"2 sampling calls (N = 2, 8) -> {runs} decode run(s)")
    assert runs < 2
    for o, s, n_alt in zip(out, solo, (2, 8)):
        _same(o, s, alternatives=True)
        _check_result(cfg, o, n_alt, False, 10)


def test_errors(setup):
    cfg, _, model, enc = setup
    prompt = _prompt(cfg)
    for bad in (-1, 9):
        with pytest.raises(ValueError):
            model.generate(enc, [prompt] * 3, return_alternatives=bad, **_kw(cfg, "greedy"))
