"""numpy reference of truncated sampling (include/fwamd.h: fw_generate_trunc; the TRUNC stage of dec_vocab.hip), and the
seeded launches tests/test_gpu_sampling_trunc_kernel.py sends through fw_test_logits_rules_trunc.  The contract, restated:

  L = {v : logp[v] > -inf} in the order (logp descending, id ascending);  S_k = the first min(k, |L|) ids (k == 0: L);
  w(v) = exp((logp[v] - max logp) / T),  Z = sum of w over S_k,  S = {v in S_k : mass of S_k in front of v < p Z} (p == 1:
  S_k; the first id always);  draw = arg-max over S of logp / T + gumbel(seed, row, step, v), lowest id on a tie.

Masses are float64 here.  The log-probs are the oracle's (OracleWhisper._process_logits, float32), the noise is
oracle.whisper._gumbel; neither is restated.  No GPU here."""
import dataclasses
import functools

import numpy as np

import logits_rules_refs as lr

KEY_TIE = 1e-4      # margin between the best two keys: device logf against numpy (tests/test_gpu_logits_rules.py)
MASS_MARGIN = 1e-2  # |mass ahead - p Z| / Z of every id of S_k: three times V 2^-24, the worst error of an fp32 sum of V terms


def order_of(lp):
    """the live ids in the order of the contract"""
    lp = np.asarray(lp)
    live = np.flatnonzero(lp > -np.inf)
    return live[np.lexsort((live, -lp[live].astype(np.float64)))]


def trunc_set(lp, k, p, inv_temp):
    """dict(order, S_k, S: ids in order; ahead, Z: the masses of S_k in float64 (None without a nucleus); margin: the smallest
    |ahead(v) - p Z| / Z over S_k, inf without a nucleus)"""
    assert k >= 0 and 0 < p <= 1
    order = order_of(lp)
    Sk = order if k == 0 else order[:min(k, order.size)]
    out = dict(order=order, S_k=Sk, S=Sk, ahead=None, Z=None, margin=float("inf"))
    if p < 1 and Sk.size:
        x = np.asarray(lp, np.float64)[Sk]
        w = np.exp((x - x[0]) * np.float64(inv_temp))
        Z = w.sum()
        ahead = np.cumsum(w) - w
        keep = ahead < p * Z
        keep[0] = True
        out.update(S=Sk[keep], ahead=ahead, Z=Z, margin=float(np.abs(ahead - p * Z).min() / Z))
    return out


def draw(lp, S, inv_temp, noise):
    """(id, gap): the arg-max over S of lp * inv_temp + noise in float32 as the existing sampling references compute it
    (lowest id on a tie), and the gap to the runner-up inside S (inf with one id); (0, inf) for an empty S"""
    if len(S) == 0:
        return 0, float("inf")
    S = np.sort(np.asarray(S))
    key = np.asarray(lp, np.float32)[S] * np.float32(inv_temp) + np.asarray(noise, np.float32)[S]
    j = int(np.argmax(key))
    rest = np.delete(key, j)
    return int(S[j]), (float(key[j] - rest.max()) if rest.size else float("inf"))


def brute_force_set(lp, k, p, inv_temp):
    """the same set by a plain Python sort and a running sum: what tests/test_sampling_trunc_host.py holds trunc_set to"""
    live = sorted((v for v in range(len(lp)) if lp[v] > -np.inf), key=lambda v: (-float(lp[v]), v))
    Sk = live if k == 0 else live[:k]
    if p == 1 or not Sk:
        return Sk
    top = float(lp[Sk[0]])
    w = [float(np.exp((float(lp[v]) - top) * float(inv_temp))) for v in Sk]
    Z = sum(w)
    S, ahead = [], 0.0
    for i, v in enumerate(Sk):
        if i == 0 or ahead < p * Z:
            S.append(v)
        ahead += w[i]
    return S


# ---- the launches ------------------------------------------------------------------------------------------------------
def vocab_cfg(vocab):
    """the vocabulary of `vocab` on a micro-sized network (the rules kernel only reads the token ids)"""
    from faster_whisper_amd import get_config
    micro = get_config("micro")
    if vocab == "micro":
        return micro
    keep = ("name", "n_mels", "d_model", "n_heads", "n_enc_layers", "n_dec_layers")
    return dataclasses.replace(get_config(vocab), **{k: getattr(micro, k) for k in keep})


@functools.lru_cache(maxsize=None)
def env(vocab):
    from faster_whisper_amd import synthetic_weights
    from oracle.whisper import OracleWhisper
    cfg = vocab_cfg(vocab)
    w = synthetic_weights(cfg, seed=5)
    return cfg, w, OracleWhisper(cfg, w)


def distinct_row(V, rng):
    """V DISTINCT multiples of 1/4096 in [0, 16), shuffled (tests/test_gpu_logits_rules.py's family)"""
    return (rng.permutation(65536)[:V].astype(np.float32) / np.float32(4096.0)).astype(np.float32)


# the placed ids' logits over a tail in [0, 4): masses 0.40, 0.26, 0.16, 0.10, 0.07 at T = 1, and a spacing at which the
# midpoints of the first, third and fifth mass at T = 1 stay 0.017 away from every cumulative mass at T = 0.5 and T = 2
PEAKS = (30.0, 29.55, 29.1, 28.65, 28.2)


def peak_ids(cfg):
    """text ids in different threads, waves and register slots"""
    return [3, 64, 130, 257, 390, 25] if cfg.n_vocab < 4096 else [3, 64, 1029, 20000, 40001, 2050]


def peaked_row(cfg, rng, peaks=PEAKS, ids=None):
    row = (rng.permutation(65536)[:cfg.n_vocab].astype(np.float32) / np.float32(16384.0)).astype(np.float32)   # [0, 4)
    row[ids or peak_ids(cfg)[:len(peaks)]] = np.asarray(peaks, np.float32)
    return row


def _mid_p(lp, k, inv_temp, j):
    """p at the midpoint of the mass of the j-th id of S_k: S = the first j + 1 ids"""
    t = trunc_set(lp, k, 0.5, inv_temp)
    w = np.diff(np.append(t["ahead"], t["Z"]))
    return float((t["ahead"][j] + 0.5 * w[j]) / t["Z"])


class Case:
    """one launch: R rows of ONE step (n tokens of history each), per-row logits, histories, limits and sampling table"""

    def __init__(self, name, cfg, logits, k, p, T, with_ts=False, hists=None, done=None, nucleus=False, **opt):
        R = len(k)
        self.name, self.cfg, self.R = name, cfg, R
        self.logits = np.ascontiguousarray(np.broadcast_to(logits, (R, cfg.n_vocab)) if np.ndim(logits) == 1 else logits, np.float32)
        self.k = np.asarray(k, np.int32)
        self.p = np.asarray(p, np.float32)
        self.T = np.asarray(T, np.float32)
        self.inv = (np.float32(1.0) / self.T).astype(np.float32)
        # calls of 1, 2, 3, .. rows: row0 is the first row of the row's call; one seed per call, the high word used too
        row0, r = [], 0
        size = 1
        while r < R:
            row0 += [r] * min(size, R - r)
            r += size
            size = size % 4 + 1
        self.row0 = np.asarray(row0, np.int32)
        self.seed = np.asarray([(int(r0) * 2654435761 + 12345) % (1 << 40) for r0 in row0], np.uint64)
        self.with_ts, self.hists, self.done, self.opt, self.nucleus = with_ts, hists, done, opt, nucleus
        self.n = len(hists[0]) if hists is not None else 0
        self.cum = (-np.arange(R, dtype=np.float32) / np.float32(8.0)).astype(np.float32)


def cases(vocab):
    cfg, _, oracle = env(vocab)
    V = cfg.n_vocab
    rng = np.random.default_rng(2024)
    out = []
    R = 64
    # ---- top-k ----
    row = distinct_row(V, rng)
    sup = lr.suppress_list(cfg)
    n_live = V - len(set(sup) | set(cfg.suppress_begin))
    ks = [1, 2, 5, n_live - 1, n_live, n_live + 1, 100000]
    out.append(Case("top-k, distinct values", cfg, row, [ks[r % 7] for r in range(R)], [1.0] * R, [1.0] * R, suppress_tokens=sup))
    # two tie groups, their ids in different threads, waves, register slots and the last, partial stride of 1024
    g1 = [5, 69, 1029, 700, V - 1]
    g2 = [V - 2, 6, 1030, 321]
    row = distinct_row(V, rng)
    row[g1], row[g2] = np.float32(20.0), np.float32(18.0)
    out.append(Case("top-k, ties straddle the cut", cfg, row, [[1, 2, 3, 4, 6, 7, 8][r % 7] for r in range(R)], [1.0] * R,
                    [[1.0, 4.0][r % 2] for r in range(R)], suppress_blank=False))
    # ---- few live ids ----
    tb = cfg.timestamp_begin
    row = distinct_row(V, rng)
    row[tb], row[tb + 1] = np.float32(3.0), np.float32(3.0)
    out.append(Case("first step with timestamps: 2 live ids", cfg, row, [[1, 1, 1, 2, 0, 1, 1, 5][r % 8] for r in range(32)],
                    [[1.0, 0.4][(r // 8) % 2] for r in range(32)], [1.0] * 32, with_ts=True, max_initial_timestamp_index=1))
    a, b, last = 40, 41, V - 1
    keep = {a, b}
    rows = np.stack([distinct_row(V, rng)] * 32)
    rows[:, a], rows[:, b] = np.float32(7.0), np.float32(7.0)
    hists = [[tb + 3, a, tb + 9, tb + 9] if r % 4 else [tb + 3, a, a, last] for r in range(32)]    # closed pair: {a, b}; {last}
    rows[7] = -np.inf                                                                            # nothing live
    out.append(Case("closed pair and a suppress list: 0, 1 and 2 live ids", cfg, rows,
                    [[1, 1, 1, 1, 1, 1, 5, 1][r % 8] for r in range(32)], [[1.0, 1.0, 0.3, 1.0][r % 4] for r in range(32)],
                    [1.0] * 32, with_ts=True, hists=hists, suppress_tokens=[t for t in range(tb) if t not in keep]))
    # ---- nucleus ----
    prow = peaked_row(cfg, rng)
    lp = oracle._process_logits(prow, [], False, None, False, 50, 1.0, 0, 0)
    ps = [_mid_p(lp, 0, 1.0, j) for j in (0, 2, 4)]          # S at T = 1: one id, three, every placed id
    out.append(Case("nucleus, peaked row, three temperatures", cfg, prow, [0] * R, [ps[r % 3] for r in range(R)],
                    [[0.5, 1.0, 2.0][(r // 3) % 3] for r in range(R)], nucleus=True, suppress_blank=False))
    # a tie group of three at the boundary: the cut falls after its first and after its second id
    trow = peaked_row(cfg, rng, peaks=(30.0, 29.5, 29.5, 29.5, 29.0))
    lp = oracle._process_logits(trow, [], False, None, False, 50, 1.0, 0, 0)
    ps = [_mid_p(lp, 0, 1.0, j) for j in (1, 2)]
    out.append(Case("nucleus, a tie group at the boundary", cfg, trow, [0] * 32, [ps[r % 2] for r in range(32)], [1.0] * 32,
                    nucleus=True, suppress_blank=False))
    # top-k and nucleus together: Z is the top-4 mass
    ps = [_mid_p(oracle._process_logits(prow, [], False, None, False, 50, 1.0, 0, 0), 4, 1.0, j) for j in (0, 2)]
    out.append(Case("top-k 4 and nucleus", cfg, prow, [4] * 32, [ps[r % 2] for r in range(32)], [1.0] * 32, nucleus=True,
                    suppress_blank=False))
    # ---- per-row state: every row its own limits, temperature, seed and history; chunk 5 is done ----
    own = [100, 164, 230, 357, 390] if V < 4096 else [100, 164, 1129, 20000, 40001]   # (no id of a history)
    rows = np.stack([peaked_row(cfg, rng, ids=own) for _ in range(16)])
    hists = lr.row_histories(cfg, 16, 4)
    kk = [0, 1, 1, 0, 2, 5, 0, 1, 0, 1, 2, 0, 3, 0, 1, 0]
    lps = [oracle._process_logits(rows[r], hists[r], False, None, True, 50, 1.3, 2, 0) for r in range(16)]
    TT = [[0.5, 1.0, 2.0][r % 3] for r in range(16)]
    pp = [1.0 if r % 4 else _mid_p(lps[r], kk[r], 1.0 / TT[r], 0) for r in range(16)]
    done = [1 if r == 5 else 0 for r in range(16)]
    out.append(Case("per-row state", cfg, rows, kk, pp, TT, hists=hists, done=done, nucleus=True, repetition_penalty=1.3,
                    no_repeat_ngram_size=2))
    return out


@functools.lru_cache(maxsize=None)
def reference(vocab):
    """per case: list over rows of dict(lp, S, tok, gap, plain_tok, margin) (None for the rows of a done chunk)"""
    from oracle.whisper import _gumbel
    cfg, _, oracle = env(vocab)
    refs = []
    for c in cases(vocab):
        mask = None
        if c.opt.get("suppress_tokens"):
            mask = np.zeros(cfg.n_vocab, dtype=bool)
            mask[list(c.opt["suppress_tokens"])] = True
        rows = []
        for r in range(c.R):
            if c.done is not None and c.done[r]:
                rows.append(None)
                continue
            lp = oracle._process_logits(c.logits[r], list(c.hists[r]) if c.hists is not None else [], c.with_ts, mask,
                                        bool(c.opt.get("suppress_blank", True)), int(c.opt.get("max_initial_timestamp_index", 50)),
                                        float(c.opt.get("repetition_penalty", 1.0)), int(c.opt.get("no_repeat_ngram_size", 0)), 0)
            t = trunc_set(lp, int(c.k[r]), float(c.p[r]), float(c.inv[r]))
            noise = _gumbel(int(c.seed[r]), r - int(c.row0[r]), c.n, cfg.n_vocab)
            tok, gap = draw(lp, t["S"], c.inv[r], noise)
            plain_tok, _ = draw(lp, t["order"], c.inv[r], noise)
            rows.append(dict(lp=lp, S=t["S"], tok=tok, gap=gap, plain_tok=plain_tok, margin=t["margin"], n_live=t["order"].size))
        refs.append(rows)
    return refs
