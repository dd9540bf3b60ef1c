"""References of the scoring tests (tests/test_score_refs.py on the CPU, tests/test_gpu_score_kernel.py and
tests/test_gpu_score.py on the GPU).  No GPU here.

  * the scoring kernel (dec_vocab.hip: dec_score_kernel) restated in float64, row by row: the raw log-softmax, or the
    decoding rules first — WHICH ids the rules forbid is asked of the oracle (oracle/whisper.py::_process_logits on the
    row's history; rule (e) included), the one float32 operation the rules contain (the repetition penalty, v * p or
    v / p once per distinct history id) is applied as the kernel's contract states it, and the log-softmax of what is
    left is taken in float64;
  * the model-level reference: ONE decoder_full pass of the oracle over prompt + targets -> logits -> the same;
  * the seeded inputs of the kernel tests.  Their rule-mode rows are built so that rule (e) is never a tie: at every
    scored row the oracle's rule margin is nan or at least MARGIN in magnitude (asserted on the CPU by
    tests/test_score_refs.py), so no row is excluded from any comparison."""
import types

import numpy as np

import logits_rules_refs as lr

SENT_F = np.float32(-4321.0)     # what the output arrays hold before a launch
SENT_I = -99
MARGIN = 1e-2                    # smallest |rule (e) margin| of any scored rule-mode row
SEEDS = (101, 102, 103, 104, 105)   # the kernel tests run every case on each of these
PLACED = 24.0                    # above every level of the signed family ([-8, 8)) and its whole mass


def _oracle_rules(cfg):
    """oracle/whisper.py::_process_logits needs only the config of its OracleWhisper: a stand-in without weights"""
    from oracle.whisper import OracleWhisper
    ns = types.SimpleNamespace(cfg=cfg)
    return ns, lambda *a: OracleWhisper._process_logits(ns, *a)


def log_softmax64(x):
    x = np.asarray(x, np.float64)
    m = x.max()
    if not np.isfinite(m):
        return np.full(x.shape, -np.inf)
    return x - (m + np.log(np.exp(x - m).sum()))


def raw_lp64(row):
    return log_softmax64(np.asarray(row, np.float32))


def rules_lp64(cfg, row, hist, with_ts, suppress_tokens=None, suppress_blank=True, max_initial_timestamp_index=50,
               repetition_penalty=1.0, no_repeat_ngram_size=0):
    """(lp64 [V], rule (e) margin as the oracle reports it) of one row after the decoding rules"""
    V = cfg.n_vocab
    row = np.array(row, np.float32)
    hist = [int(t) for t in hist]
    mask = None
    if suppress_tokens:
        mask = np.zeros(V, bool)
        mask[[t for t in suppress_tokens if 0 <= t < V]] = True
    ns, proc = _oracle_rules(cfg)
    lp32 = proc(row, hist, bool(with_ts), mask, bool(suppress_blank), max_initial_timestamp_index,
                float(repetition_penalty), int(no_repeat_ngram_size), 0)
    dead = ~np.isfinite(lp32)
    if repetition_penalty != 1.0 and hist:
        p = np.float32(repetition_penalty)
        for t in sorted(set(hist)):
            row[t] = row[t] * p if row[t] < 0 else row[t] / p
    x = row.astype(np.float64)
    x[dead] = -np.inf
    return log_softmax64(x), ns._rule_margin


def pick(lp, target):
    """(lp of the target, arg-max id with ties to the lowest id, its lp); a row with nothing left: (.., 0, -inf)"""
    best = int(np.argmax(lp))                       # (numpy returns the first of equal maxima)
    if not np.isfinite(lp[best]):
        best = 0
    return float(lp[target]), best, float(lp[best])


def score_rows_ref(cfg, logits, targets, hists=None, rules=None, with_ts=False):
    """what ONE launch through fw_test_score_rows must leave from sentinel-filled outputs: lp / best_lp float64 [rows],
    best_id [rows], margins (rule (e)'s, per scored row; nan in raw mode)"""
    R = logits.shape[0]
    out = dict(lp=np.full(R, float(SENT_F)), best_id=np.full(R, SENT_I, np.int64), best_lp=np.full(R, float(SENT_F)),
               margins=[])
    for r in range(R):
        if targets[r] < 0:
            continue
        if rules is None:
            lp, margin = raw_lp64(logits[r]), float("nan")
        else:
            lp, margin = rules_lp64(cfg, logits[r], hists[r] if hists is not None else [], with_ts, **rules)
        out["lp"][r], out["best_id"][r], out["best_lp"][r] = pick(lp, int(targets[r]))
        out["margins"].append(margin)
    return out


# ---- model level -----------------------------------------------------------------------------------------------------
def model_logits(oracle, enc_b, prompt, targets):
    """float32 logits [len(targets) + 1][V] of the positions that predict target 0 .. and the closing <eot>: ONE
    teacher-forced pass over prompt + targets"""
    import torch
    with torch.no_grad():
        enc_t = oracle._r(torch.from_numpy(np.ascontiguousarray(enc_b[None], np.float32)))
        ckv = oracle.cross_kv(enc_t)
        toks = torch.tensor([list(prompt) + [int(t) for t in targets]], dtype=torch.long)
        hid = oracle.decoder_full(toks, ckv)
        P = len(prompt)
        return oracle.logits(hid[0, P - 1:P + len(targets)]).numpy().astype(np.float32)


def model_ref(oracle, enc_b, prompt, targets, rules=None):
    """Whisper.score for one sequence on the oracle: dict(token_lp [n] float64, end_lp, best_ids [n + 1], best_lp [n + 1],
    margins [n + 1]).  rules: None (raw) or the rule keywords; the timestamp mode follows the prompt."""
    cfg = oracle.cfg
    lg = model_logits(oracle, enc_b, prompt, targets)
    seq = [int(t) for t in targets] + [cfg.eot]
    with_ts = cfg.no_timestamps not in prompt
    lps, ids, blps, margins = [], [], [], []
    for k, t in enumerate(seq):
        if rules is None:
            lp, m = raw_lp64(lg[k]), float("nan")
        else:
            lp, m = rules_lp64(cfg, lg[k], seq[:k], with_ts, **rules)
        a, b, c = pick(lp, t)
        lps.append(a); ids.append(b); blps.append(c); margins.append(m)
    return dict(token_lp=np.array(lps[:-1]), end_lp=lps[-1], best_ids=ids, best_lp=np.array(blps), margins=margins)


def cum32(values):
    """the values added in order in float32"""
    acc = np.float32(0.0)
    for v in values:
        acc = np.float32(acc + np.float32(v))
    return float(acc)


# ---- inputs of the kernel tests --------------------------------------------------------------------------------------
def edge_targets(cfg, R, rng):
    """targets of a raw launch: ids 0, V - 1 and ts_begin, rows without a target, the rest random"""
    V = cfg.n_vocab
    t = rng.integers(0, V, R).astype(np.int32)
    fixed = [0, V - 1, cfg.timestamp_begin, -1]
    for i, v in enumerate(fixed[:R]):
        t[i] = v
    if R > 8:
        t[R // 2] = -1
        t[R - 1] = -7
    return t


def raw_cases(cfg, seed):
    """(name, logits [R][V], targets [R]) of the raw-mode launches"""
    V = cfg.n_vocab
    rng = np.random.default_rng(seed)
    out = []
    for R in (1, 37):
        lg = lr.signed_rows(V, R, rng)
        t = edge_targets(cfg, R, rng) if R > 1 else np.array([int(rng.integers(0, V))], np.int32)
        out.append((f"signed rows x {R}", lg, t))
    # -inf everywhere but the target; a target whose logit is -inf; both in one launch, beside a plain row
    lg = lr.signed_rows(V, 3, rng)
    t = rng.integers(0, V, 3).astype(np.int32)
    keep = lg[0, t[0]]
    lg[0, :] = -np.inf
    lg[0, t[0]] = keep
    lg[1, t[1]] = -np.inf
    out.append(("-inf rows", lg, t))
    # exact ties for the maximum across register slots, lanes and waves: the lowest id wins
    lg = lr.tied_rows(V, 4, rng)
    tie_sets = [[5, 1024 + 5, V - 1], [1023, 1024], [63, 64, 1025], [V - 2, V - 1]]
    for r, ids in enumerate(tie_sets):
        lg[r, ids] = np.float32(PLACED)
    out.append(("tied maxima", lg, np.array([s[-1] for s in tie_sets], np.int32)))
    # magnitude 1e4, spread 1e-3 (one float32 spacing at 1e4 is 9.8e-4: the row holds two adjacent values)
    base = np.float32(1.0e4)
    step = np.spacing(base)
    lg = (base + step * rng.integers(0, 2, (3, V))).astype(np.float32)
    lg[1] = -lg[1]
    out.append(("magnitude 1e4", lg, rng.integers(0, V, 3).astype(np.int32)))
    return out


def _place(lg, r, ids, value=PLACED):
    lg[r, list(ids)] = np.float32(value)


def rule_cases(cfg, seed):
    """(name, logits [R][V], targets [R], hists [R], options, with_ts) of the rule-mode launches: every rule family of
    tests/test_gpu_logits_rules.py once, a history per row.  Where the timestamp rules are on, one id per row is PLACED
    above the rest of the row on the side rule (e) is meant to fall, so that its margin is far from zero."""
    V, tb, NT = cfg.n_vocab, cfg.timestamp_begin, cfg.n_text_ctx
    rng = np.random.default_rng(seed + 1000)
    sup = lr.suppress_list(cfg)
    out = []
    # penalty + n-gram, timestamps off: repeats, ids 0 and V - 1, both signs; targets: penalised, banned, untouched ids
    rep = [20, 21, 22, 20, 21, 23, 0, V - 1, 20, 21]
    lg = lr.spike(lr.signed_rows(V, 6, rng), (20, 0), (21, V - 1))
    hists = [rep, rep, rep[:8], [], [20, 21], [int(t) for t in 30 + rng.integers(0, 4, NT - 1)]]
    t = np.array([20, 22, 23, 5, -1, 31], np.int32)
    out.append(("penalty 1.3 + ngram 3", lg, t, hists, dict(repetition_penalty=1.3, no_repeat_ngram_size=3,
                                                          suppress_blank=False), False))
    out.append(("penalty 0.8 + ngram 2 + suppress list", lg, t, hists,
                dict(repetition_penalty=0.8, no_repeat_ngram_size=2, suppress_tokens=sup), False))
    # the first generated position: suppress-blank and the initial-timestamp limit (n = 0 on every row)
    lg = lr.signed_rows(V, 4, rng)
    t = np.array([tb, tb + 3, tb + 4, cfg.suppress_begin[0]], np.int32)     # allowed, allowed, past the limit, text
    out.append(("first position, limit 3", lg, t, [[]] * 4, dict(max_initial_timestamp_index=3), True))
    out.append(("first position, timestamps off", lg, np.array([5, cfg.suppress_begin[0], cfg.eot, V - 1], np.int32),
                [[]] * 4, dict(suppress_blank=True, suppress_tokens=sup), False))
    # open and closed pairs, text after a timestamp, the last timestamp id; rule (e) on both sides
    a = 40
    hists = [[tb + 3, a, a + 1, a],            # text after an opening timestamp: (e) text side
             [tb + 3, a, a + 1, a],            # ... (e) timestamp side
             [tb + 3, a, a, tb + 9],           # an open pair: text is forbidden
             [tb + 3, a, tb + 9, tb + 9],      # a closed pair: no timestamp
             [tb + 3, a, a, V - 1],            # the last timestamp id, open
             [tb + 1] + [a, a + 1] * ((NT - 2) // 2)]   # a long history (n = NT - 1 or NT - 2)
    lg = lr.signed_rows(V, len(hists), rng)
    _place(lg, 0, [a + 2])                     # a text id far above the timestamp mass
    _place(lg, 1, [tb + 20])                   # a timestamp far above every text id
    _place(lg, 2, [tb + 12])
    _place(lg, 3, [a + 5])
    _place(lg, 4, [cfg.eot])
    _place(lg, 5, [a + 7])
    t = np.array([a + 2, tb + 20, tb + 9, a + 5, cfg.eot, tb + 2], np.int32)
    out.append(("timestamp states", lg, t, hists, dict(suppress_tokens=sup, repetition_penalty=1.1), True))
    return out
