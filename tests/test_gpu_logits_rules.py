"""The logits-rules kernel (dec_vocab.hip: dec_logits_process_kernel — suppress lists, repetition penalty, no-repeat
n-gram, the five timestamp rules, fp32 log-softmax, top-2K candidates of cum + logp; Gumbel arg-max when sampling)
against the oracle's restatement of CTranslate2's logits processors (oracle/whisper.py::_process_logits, SURVEY.md
A.3), ONE launch on seeded random logits through the C ABI test hook fw_test_logits_rules.

The comparison is id for id: every row holds DISTINCT multiples of 1/4096, so two candidates are never closer than
2.4e-4 and the order is decided exactly; candidate values agree to float32 round-off
of the log-sum-exp.  Rule (e) (timestamp mass vs best text token) is exercised on both sides of its threshold with a
margin far above that round-off.

The second half of the file goes through fw_test_logits_rules_ex, which exposes the state of the launch (the logits row
as the sparse rules leave it, done per chunk, all 32 candidate slots of a row from sentinels), against the float64
restatement of tests/logits_rules_refs.py: signed and wide logits, ties, per-row histories, beam 16, finished chunks,
the first step's timestamp limit.  tests/test_logits_rules_refs.py shows on the CPU that each of those inputs tells the
right kernel from a subtly wrong one."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["micro", "tiny.en", "large-v3"])
def env(request):
    """a model is needed only for its config (token ids, vocabulary): decoder-less geometry is irrelevant here, so the
    large-v3 vocabulary (51 866, multilingual ids) rides on a micro-sized network.  The micro vocabulary (1 913 ids,
    timestamps from 412) takes the kernel's instantiation with the per-lane class test (TXI = 0), the two others the
    one with the compile-time split (TXI = 48)."""
    from faster_whisper_amd import Whisper, get_config, synthetic_weights
    from oracle.whisper import OracleWhisper
    import dataclasses
    full = get_config(request.param)
    micro = get_config("micro")
    keep = ("name", "n_mels", "d_model", "n_heads", "n_enc_layers", "n_dec_layers")
    cfg = dataclasses.replace(full, **{k: getattr(micro, k) for k in keep if hasattr(micro, k)})
    w = synthetic_weights(cfg, seed=5)
    model = Whisper("synthetic:rules", device="cuda", files={"config": cfg, "weights": w}, max_batch_size=2,
                    max_beam_size=16)
    return cfg, model, OracleWhisper(cfg, w)


def _logits(cfg, R, rng, scale=1.0):
    """every row: V DISTINCT multiples of 1/4096 in [0, 16) (times `scale`, a power of two), shuffled"""
    V = cfg.n_vocab
    assert V <= 65536
    base = rng.permutation(65536)[:V].astype(np.float32) / np.float32(4096.0)
    out = np.stack([rng.permutation(base) for _ in range(R)]) * np.float32(scale)
    return np.ascontiguousarray(out, dtype=np.float32)


def _launch(model, logits, hist, cum, K, with_ts, **opt):
    from faster_whisper_amd import _lib
    R, V = logits.shape
    n = len(hist[0]) if hist is not None and len(hist) else 0
    o = _lib.FwGenOpts()
    o.beam_size, o.patience, o.num_hypotheses, o.length_penalty = K, 1.0, 1, 1.0
    o.repetition_penalty = float(opt.get("repetition_penalty", 1.0))
    o.no_repeat_ngram_size = int(opt.get("no_repeat_ngram_size", 0))
    o.max_length = 448
    o.max_initial_timestamp_index = int(opt.get("max_initial_timestamp_index", 50))
    o.suppress_blank = int(opt.get("suppress_blank", True))
    sup = np.asarray(opt.get("suppress_tokens") or [], dtype=np.int32)
    o.suppress_tokens = _lib.as_i32p(sup) if sup.size else None
    o.n_suppress_tokens = int(sup.size)
    o.sampling_topk = int(opt.get("sampling_topk", 1))
    o.sampling_temperature = float(opt.get("sampling_temperature", 1.0))
    o.seed = int(opt.get("seed", 0))
    o.min_new_tokens = int(opt.get("min_new_tokens", 0))
    Cn = 1 if (K == 1 and o.sampling_topk != 1) else 2 * K
    h = np.ascontiguousarray(np.asarray(hist, dtype=np.int32).reshape(R, n)) if n else np.zeros((R, 1), np.int32)
    cv = np.zeros((R, Cn), np.float32)
    ct = np.zeros((R, Cn), np.int32)
    cum = np.ascontiguousarray(cum, dtype=np.float32)
    _lib.check(model._lib.fw_test_logits_rules(model._replicas[0].handle, _lib.ptr(logits), R, _lib.ptr(h), n,
                                               _lib.ptr(cum), C.byref(o), int(with_ts), _lib.ptr(cv), _lib.ptr(ct)))
    return cv, ct


def _reference(oracle, logits, hist, cum, K, with_ts, **opt):
    cfg = oracle.cfg
    V = logits.shape[1]
    mask = None
    if opt.get("suppress_tokens"):
        mask = np.zeros(V, dtype=bool)
        mask[[t for t in opt["suppress_tokens"] if 0 <= t < V]] = True
    vals, toks = [], []
    for r in range(logits.shape[0]):
        lp = oracle._process_logits(logits[r], list(hist[r]) if hist is not None else [], with_ts, mask,
                                    bool(opt.get("suppress_blank", True)), int(opt.get("max_initial_timestamp_index", 50)),
                                    float(opt.get("repetition_penalty", 1.0)), int(opt.get("no_repeat_ngram_size", 0)),
                                    int(opt.get("min_new_tokens", 0)))
        order = np.lexsort((np.arange(V), -lp))[:2 * K]          # value descending, index ascending
        v = np.float32(cum[r]) + lp[order]
        t = order.copy()
        dead = ~np.isfinite(lp[order])
        v[dead], t[dead] = -np.inf, 0
        vals.append(v)
        toks.append(t)
    return np.stack(vals).astype(np.float32), np.stack(toks).astype(np.int32)


def _compare(env, hist, K, with_ts, seed, scale=1.0, edit=None, **opt):
    cfg, model, oracle = env
    rng = np.random.default_rng(seed)
    R = 2 * K
    logits = _logits(cfg, R, rng, scale)
    if edit is not None:
        edit(logits)
    cum = -rng.random(R).astype(np.float32) * 3
    hist = None if hist is None else [list(hist) for _ in range(R)]
    cv, ct = _launch(model, logits, hist, cum, K, with_ts, **opt)
    rv, rt = _reference(oracle, logits, hist, cum, K, with_ts, **opt)
    assert np.array_equal(ct, rt), (ct[0], rt[0])
    fin = np.isfinite(rv)
    assert np.array_equal(np.isfinite(cv), fin)
    assert np.abs(cv[fin] - rv[fin]).max() < 2e-5
    return cv, ct


def _sup(cfg):
    return sorted({cfg.sot, cfg.sot_prev, cfg.sot_lm, cfg.no_speech, 1, 2, 7, 63, 64, 1023, 1024, cfg.n_vocab - 1})


def test_plain_and_suppress_lists(env):
    cfg = env[0]
    _compare(env, None, 5, False, 1, suppress_blank=False)
    _compare(env, None, 5, False, 2, suppress_blank=True, suppress_tokens=_sup(cfg))
    _compare(env, [11, 12, 13], 5, False, 3, suppress_tokens=_sup(cfg))
    _compare(env, [11, 12], 1, False, 4, suppress_tokens=_sup(cfg), min_new_tokens=5)   # <eot> held back
    _compare(env, [11] * 447 if cfg.n_text_ctx > 447 else [11] * (cfg.n_text_ctx - 1), 2, False, 5)   # longest history


def test_repetition_penalty_and_no_repeat_ngram(env):
    cfg = env[0]
    h = [20, 21, 22, 20, 21, 23, 20, 21]
    _compare(env, h, 5, False, 6, repetition_penalty=1.3)
    _compare(env, h, 5, False, 7, no_repeat_ngram_size=3)          # 20 21 -> 22 and 23 are forbidden
    _compare(env, h, 3, False, 8, repetition_penalty=0.8, no_repeat_ngram_size=2, suppress_tokens=_sup(cfg))
    _compare(env, [5], 5, False, 9, no_repeat_ngram_size=1)


def test_timestamp_rules(env):
    cfg = env[0]
    tb = cfg.timestamp_begin
    sup = _sup(cfg)

    def quiet_timestamps(lg):
        lg[:, tb:] -= 8.0      # timestamp mass well below the best text token: rule (e) leaves the text ids alone

    # with the raw draw the 1 501 timestamp logits outweigh the best text token (rule (e) masks the text ids)
    for K in (1, 5):
        for edit in (quiet_timestamps, None):
            _compare(env, None, K, True, 10, edit=edit, suppress_tokens=sup)             # first token: a timestamp <= tb+50
            _compare(env, None, K, True, 11, edit=edit, max_initial_timestamp_index=0)
            _compare(env, None, K, True, 12, edit=edit, max_initial_timestamp_index=-1)
            _compare(env, [tb + 3], K, True, 13, edit=edit, suppress_tokens=sup)         # after the opening timestamp: text only
            _compare(env, [tb + 3, 40], K, True, 14, edit=edit)                          # text, or timestamps > tb+3
            _compare(env, [tb + 3, 40, tb + 9], K, True, 15, edit=edit)                  # open pair: timestamp >= tb+9 or <eot>
            _compare(env, [tb + 3, 40, tb + 9, tb + 9], K, True, 16, edit=edit)          # closed pair: text only
            _compare(env, [tb + 3, 40, tb + 9, tb + 9, 41, 42], K, True, 17, edit=edit, suppress_tokens=sup)   # > tb+9


def test_timestamp_mass_rule_both_sides(env):
    """rule (e): when logsumexp(timestamp logits) > max(text logit) the text ids are masked"""
    cfg = env[0]
    tb = cfg.timestamp_begin

    def favour_text(lg):
        lg[:, 100] = lg.max() + 8.0          # one text token far above the whole timestamp mass

    def favour_timestamps(lg):
        lg[:, tb + 20:tb + 60] += 8.0        # the timestamp mass far above the best text token

    for K in (1, 5):
        _, ct = _compare(env, [tb + 3, 40], K, True, 20, edit=favour_text)
        assert (ct[:, 0] == 100).all()
        _, ct = _compare(env, [tb + 3, 40], K, True, 21, edit=favour_timestamps)
        assert (ct >= tb).all()


def test_everything_masked(env):
    """closed timestamp pair (no timestamps) + every text id and <eot> suppressed: no candidate at all"""
    cfg = env[0]
    tb = cfg.timestamp_begin
    cv, ct = _launch(env[1], _logits(cfg, 2, np.random.default_rng(3)), [[tb + 1, tb + 1]] * 2, np.zeros(2, np.float32), 1,
                     True, suppress_tokens=list(range(tb)))
    assert np.isneginf(cv).all() and (ct == 0).all()


def test_gumbel_sampling_draw(env):
    """sampling: arg-max of logp / T + Gumbel noise (counter-based hash of seed, row, step, token), recorded score =
    cum + logp of the drawn token"""
    from oracle.whisper import _gumbel
    cfg, model, oracle = env
    rng = np.random.default_rng(30)
    R, V = 4, cfg.n_vocab
    logits = _logits(cfg, R, rng, scale=0.5)
    hist = [[11, 12, 13]] * R
    cum = -rng.random(R).astype(np.float32)
    for seed, T in ((12345, 1.0), ((7 << 32) | 99, 0.7)):
        cv, ct = _launch(model, logits, hist, cum, 1, False, sampling_topk=0, sampling_temperature=T, seed=seed,
                         suppress_tokens=_sup(cfg))
        mask = np.zeros(V, dtype=bool)
        mask[_sup(cfg)] = True
        for r in range(R):
            lp = oracle._process_logits(logits[r], hist[r], False, mask, True, 50, 1.0, 0, 0)
            key = np.where(np.isfinite(lp), lp * np.float32(1.0 / T) + _gumbel(seed, r, 3, V), -np.inf)
            top2 = np.sort(key)[-2:]
            assert top2[1] - top2[0] > 1e-4, "degenerate draw in the test data"
            assert ct[r, 0] == int(np.argmax(key))
            assert abs(cv[r, 0] - (cum[r] + lp[ct[r, 0]])) < 2e-5


# ---------------------------------------------------------------------------------------------------------------------
# fw_test_logits_rules_ex against tests/logits_rules_refs.py
# ---------------------------------------------------------------------------------------------------------------------
import logits_rules_refs as lr   # noqa: E402

ABS_TOL = 2e-5               # the file's tolerance: float32 round-off of the log-sum-exp in the project's range (< 32)
SPACINGS = 10.5              # the same allowance in float32 spacings (2e-5 / 2^-19), for values outside that range


def _opts(K, **opt):
    from faster_whisper_amd import _lib
    o = _lib.FwGenOpts()
    o.beam_size, o.patience, o.num_hypotheses, o.length_penalty = K, 1.0, 1, 1.0
    o.repetition_penalty = float(opt.get("repetition_penalty", 1.0))
    o.no_repeat_ngram_size = int(opt.get("no_repeat_ngram_size", 0))
    o.max_length = 448
    o.max_initial_timestamp_index = int(opt.get("max_initial_timestamp_index", 50))
    o.suppress_blank = int(opt.get("suppress_blank", True))
    sup = np.asarray(opt.get("suppress_tokens") or [], dtype=np.int32)
    o.suppress_tokens = _lib.as_i32p(sup) if sup.size else None
    o.n_suppress_tokens = int(sup.size)
    o.sampling_topk = int(opt.get("sampling_topk", 1))
    o.sampling_temperature = float(opt.get("sampling_temperature", 1.0))
    o.seed = int(opt.get("seed", 0))
    o.min_new_tokens = int(opt.get("min_new_tokens", 0))
    return o, sup          # (sup: keeps the array the options point to alive)


def _launch_ex(model, logits, hists, cum, K, with_ts, done=None, table=None, rc_only=False, **opt):
    """one launch through fw_test_logits_rules_ex from sentinel-filled candidate arrays: dict(logits, val, tok, lp), the
    row and all 32 slots of every row as the launch leaves them.  table = (inv_temp [R], seed [R], row0 [R]) | None."""
    from faster_whisper_amd import _lib
    R, V = logits.shape
    n = len(hists[0]) if hists is not None else 0
    o, keep = _opts(K, **opt)
    h = np.ascontiguousarray(np.asarray(hists, dtype=np.int32).reshape(R, n)) if n else np.zeros((R, 1), np.int32)
    lg = np.array(logits, dtype=np.float32, order="C")
    cv = np.full((R, lr.STRIDE), lr.SENT_F, np.float32)
    cl = np.full((R, lr.STRIDE), lr.SENT_F, np.float32)
    ct = np.full((R, lr.STRIDE), lr.SENT_I, np.int32)
    cum = np.ascontiguousarray(cum, dtype=np.float32)
    dn = None if done is None else np.ascontiguousarray(done, dtype=np.int32)
    tab = [None, None, None]
    if table is not None:
        tab = [np.ascontiguousarray(table[0], np.float32), np.ascontiguousarray(table[1], np.uint64),
               np.ascontiguousarray(table[2], np.int32)]
    rc = model._lib.fw_test_logits_rules_ex(
        model._replicas[0].handle, _lib.ptr(lg), R, _lib.ptr(h), n, _lib.ptr(cum), C.byref(o), int(with_ts),
        None if dn is None else _lib.ptr(dn), *[None if t is None else _lib.ptr(t) for t in tab], _lib.ptr(cv),
        _lib.ptr(ct), _lib.ptr(cl))
    out = dict(logits=lg, val=cv, tok=ct, lp=cl)
    if rc_only:
        return rc, out
    _lib.check(rc)
    return out


def _check(cfg, got, ref, cum, what, family="signed"):
    """a launch against tests/logits_rules_refs.py::launch_ref.  Ids, the finite pattern, the sentinels and the logits
    rows are exact; values within ABS_TOL of the float64 reference in the project's range, within SPACINGS float32
    spacings (at the value) of it on the wide family; cand_val == fl32(cum + cand_lp) bit for bit.  Returns the worst
    ratio |cand_val - ref64| / spacing32(ref64)."""
    Cn = ref["C"]
    live = ref["live"]
    # rows of finished chunks: nothing written, the row as it came; live rows: the slots from C on untouched
    assert (got["tok"][~live] == lr.SENT_I).all() and (got["val"][~live] == lr.SENT_F).all() and \
        (got["lp"][~live] == lr.SENT_F).all(), what
    assert (got["tok"][:, Cn:] == lr.SENT_I).all() and (got["val"][:, Cn:] == lr.SENT_F).all() and \
        (got["lp"][:, Cn:] == lr.SENT_F).all(), what
    # the in-place edits of the row, bit for bit (the device's float32 division is the correctly rounded one)
    same = lr.bits(got["logits"]) == lr.bits(ref["logits"])
    assert same.all(), (what, np.argwhere(~same)[:8])
    if not live.any():
        return 0.0
    t, v, l = got["tok"][live, :Cn], got["val"][live, :Cn], got["lp"][live, :Cn]
    rt, rv, rl = ref["tok"][live, :Cn], ref["val"][live, :Cn], ref["lp"][live, :Cn]
    assert np.array_equal(t, rt), (what, t[0], rt[0])
    fin = np.isfinite(rv)
    assert np.array_equal(np.isfinite(v), fin) and np.array_equal(np.isfinite(l), fin), what
    assert np.isneginf(v[~fin]).all() and np.isneginf(l[~fin]).all(), what
    c32 = np.ascontiguousarray(cum, np.float32)[live][:, None]
    assert np.array_equal(lr.bits(v)[fin], lr.bits((c32 + l).astype(np.float32))[fin]), what
    if not fin.any():
        return 0.0
    dv, dl = np.abs(v[fin] - rv[fin]), np.abs(l[fin] - rl[fin])
    ratio = float((dv / lr.spacing32(rv[fin])).max())
    print(f"[V={cfg.n_vocab}] {what}: worst |cand_val - ref64| = {dv.max():.2e} = {ratio:.2f} float32 spacings at the value, "
          f"worst |cand_lp - ref64| = {dl.max():.2e}")
    if family == "wide":
        # (cand_lp is held to cand_val by the bit relation above; on its own it gets the spacing of the value it was
        #  added to: a log-prob of -1e-3 computed through a float32 sum cannot carry the spacing of 1e-3)
        assert ratio <= SPACINGS, (what, ratio)
        assert (dl <= SPACINGS * lr.spacing32(np.maximum(np.abs(rl[fin]), np.abs(rv[fin])))).all(), what
    else:
        assert max(dv.max(), dl.max()) < ABS_TOL, (what, dv.max(), dl.max())
    return ratio


def _run(env, logits, hists, cum, K, with_ts, what, family="signed", done=None, **opt):
    cfg, model, _ = env
    ref = lr.launch_ref(cfg, logits, hists, cum, K, with_ts, done=done, **opt)
    if family in ("signed", "wide"):
        assert ref["gap"] >= lr.GAP, (what, ref["gap"])          # the order is decided: a condition on the inputs
    m = np.array(ref["margins"])
    assert (np.abs(m[np.isfinite(m)]) >= lr.GAP).all(), (what, m)   # ... and so is rule (e)
    got = _launch_ex(model, logits, hists, cum, K, with_ts, done=done, **opt)
    _check(cfg, got, ref, cum, what, family)
    return got, ref


def _cum(R, seed):
    return (-np.random.default_rng(seed).random(R) * 3).astype(np.float32)


@pytest.mark.parametrize("K", [1, 5, 16])
@pytest.mark.parametrize("family", ["signed", "wide"])
def test_rules_on_signed_and_wide_logits(env, family, K):
    cfg = env[0]
    R = 2 * K
    for i, (name, hist, opt, spiked) in enumerate(lr.rule_cases(cfg, np.random.default_rng(7))):
        lg = lr.family_rows(cfg, family, R, 1000 + 16 * i + K, spiked)
        hists = None if hist is None else [hist] * R
        _run(env, lg, hists, _cum(R, i), K, False, f"{family} K={K} {name}", family, **opt)


def test_in_place_edits(env):
    """the returned rows equal the input bit for bit except at the distinct history ids (ONE float32 v * p or v / p
    each, however often the id occurs) and the banned ids (-inf).  _check compares the whole row with the reference;
    here the reference's own edits are held to exactly those ids, and the division to the correctly rounded one."""
    cfg, model, _ = env
    V = cfg.n_vocab
    hist = [20, 21, 22, 20, 21, 23, 20, 21, 0, V - 1, 20, 21]      # 20 21 -> 22, 23 and 0 are banned by the 3-gram rule
    lg = lr.family_rows(cfg, "signed", 4, 77, ((20, 0), (21, V - 1)))
    opt = dict(repetition_penalty=1.3, no_repeat_ngram_size=3)
    got, ref = _run(env, lg, [hist] * 4, _cum(4, 1), 2, False, "in-place edits", **opt)
    changed = lr.bits(got["logits"]) != lr.bits(lg)
    assert np.array_equal(np.argwhere(changed[0]).ravel(), sorted(set(hist)))
    assert (changed == changed[0]).all()
    p = np.float32(1.3)
    for t in (20, 21, V - 1):
        want = np.where(lg[:, t] < 0, lg[:, t] * p, lg[:, t] / p).astype(np.float32)
        assert np.array_equal(lr.bits(got["logits"][:, t]), lr.bits(want)), t
    assert np.isneginf(got["logits"][:, [22, 23, 0]]).all()
    assert (lg[:, 20] > 0).all() and (lg[:, 21] < 0).all()


@pytest.mark.parametrize("K", [1, 5, 16])
def test_ties(env, K):
    """cand_tok equals the (value descending, id ascending) order id for id; tied candidates carry identical bits"""
    cfg = env[0]
    tb = cfg.timestamp_begin
    R = 2 * K
    sup = lr.suppress_list(cfg)
    lg = lr.family_rows(cfg, "tied", R, 400 + K)
    for what, hists, with_ts, opt in (("tied", None, False, dict(suppress_blank=False)),
                                      ("tied, timestamps, suppress list", [[tb + 3, 40]] * R, True, dict(suppress_tokens=sup))):
        got, ref = _run(env, lg, hists, _cum(R, K), K, with_ts, f"{what} K={K}", "tied", **opt)
        for r in range(R):
            v, l = got["val"][r, :2 * K], got["lp"][r, :2 * K]
            for u in np.unique(ref["lp"][r, :2 * K]):
                same = ref["lp"][r, :2 * K] == u
                assert np.unique(lr.bits(v[same])).size == 1 and np.unique(lr.bits(l[same])).size == 1
    rng = np.random.default_rng(500 + K)
    for what, text_only, hists, with_ts, opt in (
            ("placed ties", False, None, False, dict(suppress_blank=False)),
            ("placed ties, suppress list", False, [[11]] * R, False, dict(suppress_tokens=sup)),
            ("placed ties, timestamps", True, [[tb + 3, 40]] * R, True, {})):
        pl = lr.placed_rows(cfg, R, rng, text_only)
        got, ref = _run(env, pl, hists, _cum(R, K + 1), K, with_ts, f"{what} K={K}", "tied", **opt)
        left = [t for t in lr.placed_ids(cfg, text_only) if t not in (opt.get("suppress_tokens") or [])][:2 * K]
        assert (got["tok"][:, :len(left)] == np.asarray(left)).all()          # ascending ids, then the next levels:
        rest_t, rest_v = got["tok"][:, len(left):2 * K], got["lp"][:, len(left):2 * K]
        tied = lr.bits(rest_v)[:, 1:] == lr.bits(rest_v)[:, :-1]              # ascending again inside every level
        assert (np.diff(rest_t, axis=1)[tied] > 0).all() and (np.diff(rest_v, axis=1)[~tied] < 0).all()


def _per_row(cfg, K, n, family="signed"):
    R = 3 * K
    hists = lr.row_histories(cfg, R, n, shift=K)
    lg = lr.family_rows(cfg, family, R, 600 + 10 * n + K)
    cum = _cum(R, 50 + K)
    return R, hists, lg, cum, dict(repetition_penalty=1.3, no_repeat_ngram_size=2)


@pytest.mark.parametrize("n", [4, 5])
@pytest.mark.parametrize("K", [2, 5, 16])
def test_per_row_state_and_finished_chunks(env, K, n):
    """three chunks in one launch, every row with its own history (five timestamp states in turn, other text ids in
    every row, both parity halves of the history buffer), its own cum; then the same launch with finished chunks"""
    cfg = env[0]
    R, hists, lg, cum, opt = _per_row(cfg, K, n)
    all_live, _ = _run(env, lg, hists, cum, K, True, f"per-row K={K} n={n}", **opt)
    for done in ([0, 1, 0], [1, 0, 1]):
        got, ref = _run(env, lg, hists, cum, K, True, f"per-row K={K} n={n} done={done}", done=done, **opt)
        live = ref["live"]
        assert live.sum() == K * done.count(0)
        # rows of a done chunk: the row as it came, no penalty applied (the sentinels: _check)
        assert np.array_equal(lr.bits(got["logits"][~live]), lr.bits(lg[~live]))
        assert not np.array_equal(lr.bits(all_live["logits"][~live]), lr.bits(lg[~live]))
        for k in ("logits", "val", "tok", "lp"):                # live chunks: the all-live launch, bit for bit
            assert np.array_equal(got[k][live].view(np.uint32), all_live[k][live].view(np.uint32)), k


@pytest.mark.parametrize("K", [1, 16])
def test_first_step_timestamp_limit(env, K):
    """n = 0 with timestamps: only timestamps up to ts_begin + max_initial_timestamp_index; the value has NO upper limit
    (CTranslate2 takes a size_t): from the number of timestamp ids on, and below zero, every timestamp is allowed —
    2^31 - 1 included, which int arithmetic on the raw value would wrap into "everything forbidden\""""
    cfg = env[0]
    tb = cfg.timestamp_begin
    R = 2 * K
    lg = lr.family_rows(cfg, "signed", R, 300 + K)
    cum = _cum(R, 3)
    for blank in (True, False):
        free, _ = _run(env, lg, None, cum, K, True, f"first step K={K} mits=-1", max_initial_timestamp_index=-1,
                       suppress_blank=blank)
        assert np.isfinite(free["val"][:, :2 * K]).all() and (free["tok"][:, :2 * K] >= tb).all()
        for mits in (0, 3, 50, 1500, 1501, 100000, 2 ** 31 - 1):
            got, _ = _run(env, lg, None, cum, K, True, f"first step K={K} mits={mits} blank={blank}",
                          max_initial_timestamp_index=mits, suppress_blank=blank)
            live = min(mits + 1, 2 * K)
            assert (np.isfinite(got["val"][:, :2 * K]).sum(axis=1) == live).all()
            assert np.isneginf(got["val"][:, live:2 * K]).all() and (got["tok"][:, live:2 * K] == 0).all() and \
                np.isneginf(got["lp"][:, live:2 * K]).all()
            assert (got["tok"][:, :live] >= tb).all() and (got["tok"][:, :live] - tb <= mits).all()
            if mits >= 1500:
                for k in ("val", "tok", "lp"):
                    assert np.array_equal(got[k].view(np.uint32), free[k].view(np.uint32)), (mits, k)


@pytest.mark.parametrize("K", [5, 16])
def test_few_candidates(env, K):
    """a closed pair with every text id suppressed but three, plus <eot>: 4 candidates in order, then 2K - 4 dead slots"""
    cfg = env[0]
    hist, opt, keep = lr.few_candidates_case(cfg)
    R = 2 * K
    lg = lr.family_rows(cfg, "signed", R, 800 + K)
    got, _ = _run(env, lg, [hist] * R, _cum(R, 8), K, True, f"few candidates K={K}", **opt)
    assert (np.isfinite(got["val"][:, :2 * K]).sum(axis=1) == 4).all()
    for r in range(R):
        assert got["tok"][r, :4].tolist() == sorted(keep, key=lambda t: -lg[r, t])
    assert np.isneginf(got["val"][:, 4:2 * K]).all() and (got["tok"][:, 4:2 * K] == 0).all()


@pytest.mark.parametrize("use_table", [False, True])
def test_sampling_per_row_state(env, use_table):
    """the Gumbel draw on signed logits, every row with its own history, one finished chunk: slot 0 holds the draw (the
    arg-max of lp / T + noise) and cum + its log-prob, slot 1 (-inf, 0, -inf), slots 2 .. 31 the sentinel"""
    from oracle.whisper import _gumbel
    cfg, model, _ = env
    V, R, n = cfg.n_vocab, 6, 4
    hists = lr.row_histories(cfg, R, n)
    lg = lr.family_rows(cfg, "signed", R, 900)
    cum = _cum(R, 9)
    done = [0, 0, 1, 0, 0, 0]
    opt = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, sampling_topk=0)
    if use_table:       # rows of three calls, as in a merged sampling run
        seeds, inv_t, row0 = [5, 5, (9 << 32) | 4, (9 << 32) | 4, 77, 77], [1.0, 1.0, 2.0, 2.0, 0.5, 0.5], [0, 0, 2, 2, 4, 4]
        table = (inv_t, seeds, row0)
    else:
        seeds, inv_t, row0, table = [(7 << 32) | 99] * R, [1.0 / 0.7] * R, [0] * R, None
        opt.update(sampling_temperature=0.7, seed=seeds[0])
    inv_t = np.asarray(inv_t, np.float32) if use_table else np.full(R, np.float32(1.0) / np.float32(0.7), np.float32)
    noise = np.stack([_gumbel(seeds[r], r - row0[r], n, V) for r in range(R)])
    ref = lr.launch_ref(cfg, lg, hists, cum, 1, True, done=done, noise=noise, inv_temp=inv_t, **opt)
    assert ref["gap"] > 1e-4, "degenerate draw in the test data"
    got = _launch_ex(model, lg, hists, cum, 1, True, done=done, table=table, **opt)
    _check(cfg, got, ref, cum, f"sampling table={use_table}")
    assert (got["tok"][ref["live"], 1] == 0).all() and np.isneginf(got["val"][ref["live"], 1]).all()


def test_hook_refuses_a_wrong_test(env):
    """a history id outside the vocabulary (the sparse rules would index the row with it), a done flag that is not
    0 / 1, rows that are no multiple of the beam: FW_EINVAL before anything is launched, outputs still the sentinel"""
    from faster_whisper_amd import _lib
    cfg, model, _ = env
    V = cfg.n_vocab
    lg = lr.family_rows(cfg, "signed", 4, 1)
    cum = np.zeros(4, np.float32)
    ok = [[3, 4, 5]] * 4
    bad_hist = [[3, 4, 5], [3, V, 5], [3, 4, 5], [3, 4, 5]]
    neg_hist = [[3, 4, 5], [3, 4, 5], [3, 4, -1], [3, 4, 5]]
    for what, kw in (("id == V", dict(hists=bad_hist, K=2)), ("negative id", dict(hists=neg_hist, K=2)),
                     ("done = 2", dict(hists=ok, K=2, done=[0, 2])), ("done = -1", dict(hists=ok, K=2, done=[-1, 0])),
                     ("R % K", dict(hists=ok, K=3))):
        rc, out = _launch_ex(model, lg, kw["hists"], cum, kw["K"], False, done=kw.get("done"), rc_only=True,
                             repetition_penalty=1.3)
        assert rc == _lib.FW_EINVAL, (what, rc)
        assert (out["tok"] == lr.SENT_I).all() and (out["val"] == lr.SENT_F).all() and (out["lp"] == lr.SENT_F).all()
        assert np.array_equal(lr.bits(out["logits"]), lr.bits(lg)), what
    # the three older hooks share the body and with it the history check
    for hist in (bad_hist, neg_hist):
        with pytest.raises(ValueError):
            _launch(model, lg, hist, cum, 2, False, repetition_penalty=1.3)
    rc, _ = _launch_ex(model, lg, ok, cum, 2, False, done=[0, 1], rc_only=True, repetition_penalty=1.3)
    assert rc == 0
