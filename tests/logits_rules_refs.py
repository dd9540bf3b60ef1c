"""numpy references of tests/test_gpu_logits_rules.py and tests/test_logits_rules_refs.py: the logits rules of a decode
step in float64, the top-2K order, float32 spacing, and the seeded input families and histories the GPU
tests launch.  Written from the survey, not from the oracle: tests/test_logits_rules_refs.py holds the two restatements
against each other.  No GPU here."""
import numpy as np

SENT_F = -1234.0            # what every candidate slot holds before a launch (floats)
SENT_I = -77                # ... and the id slots
STRIDE = 32                 # candidate slots per row (dec_vocab.hip: 2 K at max_beam = 16)
GAP = 2.4e-4                # smallest gap the distinct families must leave among a row's best 2K + 1 values


def spacing32(g):
    """float32 spacing at |g|: 2^(floor(log2 |g|) - 23), and 2^-149 (the subnormal spacing) below 2^-126"""
    g = np.abs(np.asarray(g, np.float64))
    _, e = np.frexp(g)                                          # |g| = m 2^e, m in [0.5, 1); frexp(0) = (0, 0)
    return np.ldexp(1.0, np.where(g > 0, np.maximum(e - 24, -149), -149))


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


# ---- the rules ---------------------------------------------------------------------------------------------------
def timestamp_state(cfg, hist):
    """(a_hi, b_hi) of timestamp rules (b) - (d) for a history: ids below a_hi and timestamps in [ts_begin, b_hi) are
    forbidden.  What differs between the states the per-row tests cycle through."""
    tb, n = cfg.timestamp_begin, len(hist)
    last_ts = n >= 1 and hist[-1] >= tb
    penult_ts = n < 2 or hist[-2] >= tb
    a_hi, b_hi = 0, tb
    seen = [t for t in hist if t >= tb]
    if seen:
        b_hi = seen[-1] if (last_ts and not penult_ts) else seen[-1] + 1
    if last_ts:
        if penult_ts:
            b_hi = cfg.n_vocab
        else:
            a_hi = cfg.eot
    if n == 0:
        a_hi = tb
    return a_hi, b_hi


def rules_ref64_full(cfg, logits_row, hist, with_ts, suppress=None, suppress_blank=True, mits=50, rep_pen=1.0, ngram=0,
                     min_new=0, neg_div=False):
    """(row32, lp64, margin): the row as the two sparse rules leave it (float32 by contract: ONE v * p or v / p per
    distinct history id, -inf for an n-gram ban), the processed log-probs in float64 (-inf where masked), and rule (e)'s
    margin logsumexp(timestamps) - max(text) (nan when either side is empty or timestamps are off).
    neg_div: the DEFECT v / p for negative v too (tests/test_logits_rules_refs.py: the penalty case tells it apart)"""
    V = cfg.n_vocab
    row = np.array(logits_row, dtype=np.float32)
    assert row.shape == (V,)
    hist = [int(t) for t in hist]
    n = len(hist)
    if rep_pen != 1.0 and n:
        p = np.float32(rep_pen)
        for t in sorted(set(hist)):
            v = row[t]
            row[t] = v * p if (v < 0 and not neg_div) else v / p
    if ngram > 0 and n + 1 >= ngram:
        k = ngram
        tail = hist[n - (k - 1):] if k > 1 else []
        for s in range(0, n - k + 1):
            if hist[s:s + k - 1] == tail:
                row[hist[s + k - 1]] = -np.inf
    x = row.astype(np.float64)
    dead = np.zeros(V, dtype=bool)
    if suppress_blank and n == 0:
        dead[list(cfg.suppress_begin)] = True
    if suppress is not None:
        dead[[t for t in suppress if 0 <= t < V]] = True
    if n < min_new:
        dead[cfg.eot] = True
    tb = cfg.timestamp_begin
    if with_ts:
        a_hi, b_hi = timestamp_state(cfg, hist)
        dead[cfg.no_timestamps] = True                                  # (a)
        dead[:a_hi] = True                                              # (b) open pair / (d) first step
        dead[tb:b_hi] = True                                            # (b) closed pair, (c) no way back
        if n == 0 and mits is not None and mits >= 0:                   # (d): no upper limit on the value itself
            dead[min(tb + int(mits) + 1, V):] = True
    x[dead] = -np.inf
    margin = float("nan")
    if with_ts:
        ts, text = x[tb:], x[:tb]
        if np.isfinite(ts.max()) and np.isfinite(text.max()):
            margin = float(ts.max() + np.log(np.exp(ts - ts.max()).sum()) - text.max())
            if margin > 0:                                              # (e)
                x[:tb] = -np.inf
        # (one side empty: -inf > finite is false, finite > -inf masks ids that are masked already)
    m = x.max()
    if not np.isfinite(m):
        return row, np.full(V, -np.inf), margin
    return row, x - (m + np.log(np.exp(x - m).sum())), margin


def rules_ref64(cfg, logits_row, hist, with_ts, suppress, suppress_blank, mits, rep_pen, ngram, min_new):
    row, lp, _ = rules_ref64_full(cfg, logits_row, hist, with_ts, suppress, suppress_blank, mits, rep_pen, ngram, min_new)
    return row, lp


def top_ref(lp, cum, K, order="id"):
    """the first 2K of (value descending, id ascending): (cum + lp [2K] float64, ids [2K], lp [2K]); dead slots are
    (-inf, 0, -inf).  order = "highest" / "thread": the two natural WRONG tie-breaks (highest id first; thread
    id % 1024 first, then register slot id // 1024) — tests/test_logits_rules_refs.py shows the inputs tell them apart."""
    V = lp.shape[0]
    ids = np.arange(V)
    if order == "id":
        idx = np.lexsort((ids, -lp))
    elif order == "highest":
        idx = np.lexsort((-ids, -lp))
    else:
        assert order == "thread"
        idx = np.lexsort((ids // 1024, ids % 1024, -lp))
    idx = idx[:2 * K]
    sel = lp[idx].copy()
    tok = idx.astype(np.int64)
    dead = ~np.isfinite(sel)
    tok[dead] = 0
    sel[dead] = -np.inf
    if idx.size < 2 * K:                                                # (a vocabulary below 2K ids: not used here)
        pad = 2 * K - idx.size
        tok, sel = np.concatenate([tok, np.zeros(pad, np.int64)]), np.concatenate([sel, np.full(pad, -np.inf)])
    return np.float64(np.float32(cum)) + sel, tok.astype(np.int32), sel


def top_gap(lp, K):
    """smallest gap among the best 2K + 1 finite values of a row (inf with fewer than two)"""
    s = np.sort(lp[np.isfinite(lp)])[::-1][:2 * K + 1]
    return float(np.min(s[:-1] - s[1:])) if s.size >= 2 else float("inf")


# ---- input families (seeded, per row) ----------------------------------------------------------------------------
def _grid_rows(V, R, rng, step, lo):
    assert V <= 65536
    base = (rng.permutation(65536)[:V].astype(np.float64) * step + lo).astype(np.float32)
    return np.ascontiguousarray(np.stack([rng.permutation(base) for _ in range(R)]), dtype=np.float32)


def signed_rows(V, R, rng):
    """V DISTINCT multiples of 1/4096 in [-8, 8)"""
    return _grid_rows(V, R, rng, 1.0 / 4096, -8.0)


def wide_rows(V, R, rng):
    """V DISTINCT multiples of 1/256 in [-128, 128): nearly every exponential underflows"""
    return _grid_rows(V, R, rng, 1.0 / 256, -128.0)


def tied_rows(V, R, rng):
    """iid multiples of 1/4 in [-8, 8): 64 levels"""
    return np.ascontiguousarray(rng.integers(0, 64, (R, V)).astype(np.float32) / np.float32(4.0) - np.float32(8.0))


FAMILY_SHIFT = {"signed": 16.0, "wide": 256.0}           # the "all-negative" rows: [-24, -8) and [-384, -128)
FAMILIES = {"signed": signed_rows, "wide": wide_rows, "tied": tied_rows}
PLACED = 24.0               # above every level of the tied family AND above its whole timestamp mass (~ 12.5)


def placed_ids(cfg, text_only):
    """slot, lane, wave and thread boundaries of id = tid + 1024 i, clipped to the vocabulary (text_only: to the ids
    below <eot>, whose last one is added).  The micro vocabulary (1 913 ids, 400 of them text) gets the boundaries that
    exist at its size."""
    V = cfg.n_vocab
    base = [0, 63, 64, 1023, 1024, 1025, 2047, 2048, 16383, 16384, V - 1]
    if V < 4096:
        base = [0, 63, 64, 255, 256, 399, 1023, 1024, 1025, V - 1]
    hi = cfg.eot if text_only else V
    ids = sorted({t for t in base if t < hi})
    if text_only:
        ids = sorted(set(ids) | {cfg.eot - 1})
    return ids


def placed_rows(cfg, R, rng, text_only):
    """the tied family with ONE value above everything else at exactly placed_ids"""
    lg = tied_rows(cfg.n_vocab, R, rng)
    lg[:, placed_ids(cfg, text_only)] = np.float32(PLACED)
    return lg


def spike(lg, hi_ids, lo_ids):
    """per row, swap the largest values into hi_ids and the smallest into lo_ids (distinct values stay distinct): the
    history ids of the penalty / n-gram cases then sit at the top of the row and on both sides of zero"""
    for r in range(lg.shape[0]):
        order = np.argsort(lg[r])
        for j, t in enumerate(hi_ids):
            s = order[-1 - j]
            lg[r, [t, s]] = lg[r, [s, t]]
            order = np.argsort(lg[r])
        for j, t in enumerate(lo_ids):
            s = order[j]
            lg[r, [t, s]] = lg[r, [s, t]]
            order = np.argsort(lg[r])
    return lg


# ---- per-row histories -------------------------------------------------------------------------------------------
N_STATES = 5


def state_history(cfg, state, n, r):
    """history of length n (4 or 5) of row r in timestamp state `state`; the text ids differ row by row and repeat
    inside the row where the state leaves room, so the penalty and the n-gram rule act on other ids in every row"""
    tb = cfg.timestamp_begin
    last = cfg.n_vocab - 1                      # the last timestamp id
    a, b = 40 + 3 * r, 41 + 3 * r
    assert b + 1 < cfg.eot and n in (4, 5)
    h = [[tb + 3, a, b, a],                     # text after an opening timestamp
         [tb + 3, a, a, tb + 9],                # an open pair
         [tb + 3, a, tb + 9, tb + 9],           # a closed pair
         [tb + 3, a, a, last],                  # the last timestamp id, open: only it or <eot> is left
         [last, last, a, b]][state]             # ... closed and followed by text: no timestamp is left
    if n == 5:                                  # one more leading token: the same state, the other parity half
        h = ([tb + 1] if state < 4 else [last]) + h
    return h


def row_histories(cfg, R, n, shift=0):
    return [state_history(cfg, (r + shift) % N_STATES, n, r) for r in range(R)]


# ---- one launch, restated ----------------------------------------------------------------------------------------
def suppress_list(cfg):
    """the suppress list of tests/test_gpu_logits_rules.py: specials, small ids, lane / wave / slot boundaries, the last id"""
    return sorted({cfg.sot, cfg.sot_prev, cfg.sot_lm, cfg.no_speech, 1, 2, 7, 63, 64, 1023, 1024, cfg.n_vocab - 1})


def launch_ref(cfg, logits, hists, cum, K, with_ts, done=None, noise=None, inv_temp=None, defect=None, **opt):
    """what ONE launch of the rules kernel through fw_test_logits_rules_ex must leave, from buffers that start as
    sentinels: logits [R][V] float32 (bit for bit), tok [R][32], val / lp [R][32] float64 (SENT where the launch writes
    nothing: slots from C on, every slot of a done chunk's rows).  hists: one history per row (or None: n = 0), done
    [R / K] | None.  noise [R][V] + inv_temp [R]: the sampling form (K = 1): slot 0 = arg-max of lp * inv_temp + noise,
    slot 1 = (-inf, 0, -inf).  Also: gap (smallest top-(2K + 1) gap over the live rows; sampling: between the best two
    keys), margins (rule (e)'s, per live row).
    defect: None | "highest" | "thread" (tie-breaks), "row0" (every row reads row 0's history), "done" (done ignored),
    "negdiv" (v / p for negative v) — the wrong kernels the tests must tell from the right one."""
    R, V = logits.shape
    assert V == cfg.n_vocab and (done is None or R % K == 0) and R <= 48
    sampling = noise is not None
    C = 2 if sampling else 2 * K
    out = dict(logits=np.array(logits, np.float32), tok=np.full((R, STRIDE), SENT_I, np.int32),
               val=np.full((R, STRIDE), SENT_F, np.float64), lp=np.full((R, STRIDE), SENT_F, np.float64),
               live=np.ones(R, bool), C=C, gap=float("inf"), margins=[])
    order = defect if defect in ("highest", "thread") else "id"
    for r in range(R):
        if done is not None and done[r // K] and defect != "done":
            out["live"][r] = False
            continue
        h = [] if hists is None else list(hists[0 if defect == "row0" else r])
        row, lp, margin = rules_ref64_full(
            cfg, logits[r], h, with_ts, opt.get("suppress_tokens"), bool(opt.get("suppress_blank", True)),
            opt.get("max_initial_timestamp_index", 50), float(opt.get("repetition_penalty", 1.0)),
            int(opt.get("no_repeat_ngram_size", 0)), int(opt.get("min_new_tokens", 0)), neg_div=defect == "negdiv")
        out["logits"][r] = row
        out["margins"].append(margin)
        c = np.float64(np.float32(cum[r]))
        if sampling:
            key = np.where(np.isfinite(lp), lp * np.float64(np.float32(inv_temp[r])) + noise[r].astype(np.float64), -np.inf)
            best = int(np.argmax(key))
            top2 = np.sort(key)[-2:]
            out["tok"][r, :2] = (best, 0)
            out["val"][r, :2] = (c + lp[best], -np.inf)
            out["lp"][r, :2] = (lp[best], -np.inf)
            out["gap"] = min(out["gap"], float(top2[1] - top2[0]))
            continue
        v, t, l = top_ref(lp, cum[r], K, order)
        out["tok"][r, :C], out["val"][r, :C], out["lp"][r, :C] = t, v, l
        out["gap"] = min(out["gap"], top_gap(lp, K))
    return out


def rule_cases(cfg, rng):
    """(name, history or None, options, (ids that get the row's largest values, ... its smallest[, all-negative])) of the "rules on
    signed and wide logits" cases; timestamps off.  The spiked ids put the history at the top of the row and on both
    sides of zero, so the penalty and the bans change the candidates, not only the row."""
    V = cfg.n_vocab
    sup = suppress_list(cfg)
    rep = [20, 21, 22, 20, 21, 23, 0, V - 1]                      # repeats; ids 0 and V - 1
    ng = [20, 21, 22, 20, 21, 23, 20, 21]                         # 20 21 -> 22 and 23
    long_ = [int(t) for t in 30 + rng.integers(0, 4, cfg.n_text_ctx - 1)]   # the longest history, a 4-letter alphabet
    return [
        ("plain", None, dict(suppress_blank=False), ((), ())),
        ("blank", None, dict(suppress_blank=True), (tuple(cfg.suppress_begin), ())),
        ("suppress", [11, 12, 13], dict(suppress_tokens=sup), ((1, 64), (1024 if V > 1024 else 7,))),
        ("penalty 1.3", rep, dict(repetition_penalty=1.3), ((20, 0), (21, V - 1))),
        ("penalty 0.8", rep, dict(repetition_penalty=0.8), ((20, 0), (21, V - 1))),
        # the whole row below zero (shifted down by the family's width): the best ids are penalised by v * p, and
        # the log-sum-exp has a negative class maximum
        ("penalty 1.3, all-negative row", rep, dict(repetition_penalty=1.3), ((20, 0), (21, V - 1), True)),
        ("ngram 1", ng, dict(no_repeat_ngram_size=1), ((20, 22), (21, 23))),
        ("ngram 2", ng, dict(no_repeat_ngram_size=2), ((20, 22), (21, 23))),
        ("ngram 3", ng, dict(no_repeat_ngram_size=3), ((20, 22), (21, 23))),
        ("longest history, ngram 3 + penalty", long_, dict(no_repeat_ngram_size=3, repetition_penalty=1.3),
         ((30, 31), (32, 33))),
        ("ngram 4 on a history of 2 (inactive)", [20, 21], dict(no_repeat_ngram_size=4), ((20, 22), (21,))),
        ("min_new_tokens", [11, 12], dict(min_new_tokens=5), ((cfg.eot,), ())),
    ]


def family_rows(cfg, family, R, seed, spiked=((), ())):
    rng = np.random.default_rng(seed)
    lg = FAMILIES[family](cfg.n_vocab, R, rng)
    if spiked[0] or spiked[1]:
        spike(lg, spiked[0], spiked[1])
    if len(spiked) > 2 and spiked[2]:
        lg -= np.float32(FAMILY_SHIFT[family])                  # exact: every value stays a multiple of the grid step
    return lg


def few_candidates_case(cfg):
    """a closed pair with every text id suppressed but three, plus <eot>: (history, options, the 4 ids left)"""
    tb = cfg.timestamp_begin
    keep = [3, 64, cfg.eot - 1, cfg.eot]
    return [tb + 3, 40, tb + 9, tb + 9], dict(suppress_tokens=[t for t in range(tb) if t not in keep]), keep
