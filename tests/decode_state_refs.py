"""Plain numpy references of the decode-state kernels (no GPU, no torch): the per-chunk beam update
(dec_kernels.hip K19/K20), the token + position embedding (K12) and the device part of align's post-processing
(decoder.hip: align_stats_kernel, align_filter_kernel).  tests/test_decode_state_refs.py checks the references
themselves on the CPU (brute-force beam enumeration, the oracle's median filter, torch half addition);
tests/test_gpu_decode_state.py compares the kernels with them through the hooks of include/fwamd_test.h.

The beam update works on the WHOLE state as the hook fw_test_dec_beam_update returns it (both parity halves of the
token history, the KV-slot table and cum), so a test asserts what a step wrote and that it wrote nothing else."""
import numpy as np

FIN_CAP = 48          # dec_kernels.h: finished hypotheses kept per chunk


def beam_state(B, K, NT, step, P, hist, kvidx, cum, sentinel_i, sentinel_f, done=None, n_done=0, n_fin=None, fin=None):
    """the state one launch starts from, laid out as fw_test_dec_beam_update lays it out: hist [R][step], kvidx
    [R][P - 1 + step], cum [R] in parity half step & 1, the sentinels everywhere else.  fin = (fin_tok, fin_len,
    fin_score, fin_cum) as they stand, or None for sentinel-filled arrays."""
    R, cur, pos = B * K, step & 1, P - 1 + step
    st = {
        "hist2": np.full((2, R, NT), sentinel_i, np.int32),
        "kvidx2": np.full((2, R, NT), sentinel_i & 0xFF, np.uint8),
        "cum2": np.full((2, R), sentinel_f, np.float32),
        "cur_tok": np.full(R, sentinel_i, np.int32),
        "done": np.zeros(B, np.int32) if done is None else np.array(done, np.int32),
        "n_done": np.array([n_done], np.int32),
        "n_fin": np.zeros(B, np.int32) if n_fin is None else np.array(n_fin, np.int32),
    }
    if step:
        st["hist2"][cur, :, :step] = np.asarray(hist, np.int32).reshape(R, step)
    if pos:
        st["kvidx2"][cur, :, :pos] = np.asarray(kvidx, np.uint8).reshape(R, pos)
    st["cum2"][cur] = np.asarray(cum, np.float32)
    if fin is None:
        st["fin_tok"] = np.full((B, FIN_CAP, NT), sentinel_i, np.int32)
        st["fin_len"] = np.full((B, FIN_CAP), sentinel_i, np.int32)
        st["fin_score"] = np.full((B, FIN_CAP), sentinel_f, np.float32)
        st["fin_cum"] = np.full((B, FIN_CAP), sentinel_f, np.float32)
    else:
        for name, a, dt in zip(("fin_tok", "fin_len", "fin_score", "fin_cum"), fin,
                               (np.int32, np.int32, np.float32, np.float32)):
            st[name] = np.array(a, dt)
    return st


def beam_update_ref(state, cand_val, cand_tok, *, K, P, step, budget, max_fin, lp_pow, eot):
    """One beam-update step on `state` (beam_state's layout; not modified).  Returns the new state; fin_score is
    float64 there (entries recorded by this step are cum / max(len, 1) ** lp_pow in fp64, the others the input's).

    Contract, per chunk (it is oracle/whisper.py::_generate_one's beam loop, stated on the device's data):
      * a chunk that is `done` on entry is left alone, every byte of it;
      * merge: the first 2K of the chunk's finite candidates ordered by value descending, then flat index (row, then
        rank within the row) ascending; -inf candidates are never selected; at step 0 only row 0 is a source.  Rows
        arrive sorted (value descending, -inf at the tail), as the logits-rules kernel leaves them;
      * walk the first K merged slots: <eot>, or any token on the last step (step + 1 >= budget), is a finished
        hypothesis (history, plus the token unless it is <eot>; cum; score) — recorded while fewer than FIN_CAP are held;
        off the last step the slot is refilled by the next secondary (slots K ..) that is not <eot>: <eot> secondaries
        are skipped and NOT recorded;
      * the chunk finishes on the last step, with n_fin >= max_fin, or with no live beam: done = 1, n_done += 1, and
        no row state is rewritten;
      * otherwise dead beams (fewer than K live) take parent and token of live beam 0 with cum = -inf, and for every
        row k the history (parent's, plus the token at `step`), the slot table (parent's, plus the parent byte at
        P - 1 + step), cum and cur_tok go to the OTHER parity half."""
    s = {k: np.array(v, copy=True) for k, v in state.items()}
    s["fin_score"] = s["fin_score"].astype(np.float64)
    cand_val = np.asarray(cand_val, np.float32)
    cand_tok = np.asarray(cand_tok, np.int32)
    R, NT = s["hist2"].shape[1:]
    B, C = R // K, 2 * K
    assert cand_val.shape == (R, C) and cand_tok.shape == (R, C) and R == B * K
    assert not np.isnan(cand_val).any() and not (cand_val == np.inf).any()
    assert (cand_val[:, :-1] >= cand_val[:, 1:]).all(), "candidate rows must be sorted, value descending"
    cur, nxt, pos = step & 1, (step & 1) ^ 1, P - 1 + step
    last_step = step + 1 >= budget
    for c in range(B):
        if state["done"][c]:
            continue
        nsrc = 1 if step == 0 else K
        flat_v = cand_val[c * K:c * K + nsrc].reshape(-1)
        flat_t = cand_tok[c * K:c * K + nsrc].reshape(-1)
        order = [int(i) for i in np.argsort(-flat_v, kind="stable") if flat_v[i] != -np.inf][:C]
        nf = int(s["n_fin"][c])
        sec, live = K, []
        for slot in range(K):
            if slot >= len(order):
                break
            j = order[slot]
            if flat_t[j] == eot or last_step:
                if nf < FIN_CAP:
                    toks = list(state["hist2"][cur, c * K + j // C, :step])
                    if flat_t[j] != eot:
                        toks.append(int(flat_t[j]))
                    s["fin_tok"][c, nf, :len(toks)] = toks
                    s["fin_len"][c, nf] = len(toks)
                    s["fin_cum"][c, nf] = flat_v[j]
                    sc = float(flat_v[j])
                    if lp_pow != 0:
                        sc = sc / float(max(len(toks), 1)) ** float(lp_pow)
                    s["fin_score"][c, nf] = sc
                    nf += 1
                if last_step:
                    continue
                while sec < len(order) and flat_t[order[sec]] == eot:
                    sec += 1
                if sec >= len(order):
                    sec += 1
                    continue
                j = order[sec]
                sec += 1
            live.append((j // C, int(flat_t[j]), flat_v[j]))
        s["n_fin"][c] = nf
        if last_step or nf >= max_fin or not live:
            s["done"][c] = 1
            s["n_done"][0] += 1
            continue
        while len(live) < K:
            live.append((live[0][0], live[0][1], np.float32(-np.inf)))
        for k, (par, tok, cv) in enumerate(live):
            src, dst = c * K + par, c * K + k
            s["hist2"][nxt, dst, :step] = state["hist2"][cur, src, :step]
            s["hist2"][nxt, dst, step] = tok
            s["kvidx2"][nxt, dst, :pos] = state["kvidx2"][cur, src, :pos]
            s["kvidx2"][nxt, dst, pos] = par
            s["cum2"][nxt, dst] = cv
            s["cur_tok"][dst] = tok
    return s


def finished_list(state, c):
    """[(tokens, cum, score)] of chunk c in finishing order"""
    n = int(state["n_fin"][c])
    return [(list(map(int, state["fin_tok"][c, i, :state["fin_len"][c, i]])), float(state["fin_cum"][c, i]),
             float(state["fin_score"][c, i])) for i in range(n)]


# ---------------------------------------------------------------- a toy language model that drives the beam update
def toy_table(seed, V, n=None):
    """log-softmax rows of a seeded normal table [V + 1][V] (or [n][V + 1][V]), float32"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(((V + 1, V) if n is None else (n, V + 1, V))) * 1.5
    return (x - np.log(np.exp(x).sum(axis=-1, keepdims=True))).astype(np.float32)


def toy_candidates(logp, state, B, K, step, done=None):
    """cand_val / cand_tok [B * K][2K] of the toy model logp [V + 1][V] (row V: the start symbol; row t: after token
    t): per row the top 2K of fp32 cum + logp[prev], value descending then token ascending; -inf (token 0) where the
    vocabulary has fewer than 2K tokens, on dead rows (cum = -inf) and on chunks that are done.  logp [B][V + 1][V]
    gives every chunk its own table."""
    R, C = B * K, 2 * K
    logp = np.asarray(logp, np.float32)
    if logp.ndim == 2:
        logp = np.broadcast_to(logp, (B,) + logp.shape)
    V = logp.shape[-1]
    cur = step & 1
    val = np.full((R, C), -np.inf, np.float32)
    tok = np.zeros((R, C), np.int32)
    for r in range(R):
        c = r // K
        if done is not None and done[c]:
            continue
        prev = V if step == 0 else int(state["hist2"][cur, r, step - 1])
        cum = state["cum2"][cur, r]
        v = (np.float32(cum) + logp[c, prev]).astype(np.float32)
        order = np.argsort(-v, kind="stable")[:C]
        order = [int(i) for i in order if v[i] != -np.inf]
        val[r, :len(order)] = v[order]
        tok[r, :len(order)] = order
    return val, tok


def chain_inputs(state, B, K, P, step):
    """what the next launch takes from the previous one's output: hist [R][step], kvidx [R][P - 1 + step], cum [R] of
    parity half step & 1.  Chunks that are done wrote nothing there (it holds the sentinel): they get zeros, which no
    launch reads."""
    cur, pos = step & 1, P - 1 + step
    live = np.repeat(np.asarray(state["done"]) == 0, K)
    hist = np.where(live[:, None], state["hist2"][cur, :, :step], 0).astype(np.int32)
    kvidx = np.where(live[:, None], state["kvidx2"][cur, :, :pos], 0).astype(np.uint8)
    cum = np.where(live, state["cum2"][cur], np.float32(0)).astype(np.float32)
    return hist, kvidx, cum


def run_chain(logp, B, K, NT, P, budget, max_fin, lp_pow, eot, sentinel_i=-77, sentinel_f=-1234.5, step_fn=None):
    """beam search over the toy model: beam_update_ref (or step_fn(state, cand_val, cand_tok, step) -> state, e.g. the
    kernel) chained until every chunk is done.  Every step starts from a freshly laid-out state (beam_state) built from
    the previous output, exactly what a chain of hook calls does.  Returns the final state."""
    R = B * K
    st = beam_state(B, K, NT, 0, P, None, np.zeros((R, P - 1), np.uint8), np.zeros(R, np.float32), sentinel_i,
                    sentinel_f)
    for step in range(budget):
        cv, ct = toy_candidates(logp, st, B, K, step, st["done"])
        if step_fn is None:
            out = beam_update_ref(st, cv, ct, K=K, P=P, step=step, budget=budget, max_fin=max_fin, lp_pow=lp_pow,
                                  eot=eot)
        else:
            out = step_fn(st, cv, ct, step)
        if out["done"].all():
            return out
        hist, kvidx, cum = chain_inputs(out, B, K, P, step + 1)
        st = beam_state(B, K, NT, step + 1, P, hist, kvidx, cum, sentinel_i, sentinel_f, done=out["done"],
                        n_done=int(out["n_done"][0]), n_fin=out["n_fin"],
                        fin=(out["fin_tok"], out["fin_len"], out["fin_score"], out["fin_cum"]))
    raise AssertionError("the chain did not finish within its budget")


# ---------------------------------------------------------------- embedding
def embed_ref(tok, emb, pos_emb, pos):
    """fp16(fp32(E[tok[r]]) + fp32(pos_emb[pos[r]])) as float32; emb / pos_emb are rounded to fp16 first (the hook does)"""
    e = np.asarray(emb, np.float32).astype(np.float16).astype(np.float32)
    p = np.asarray(pos_emb, np.float32).astype(np.float16).astype(np.float32)
    return (e[np.asarray(tok)] + p[np.asarray(pos)]).astype(np.float16).astype(np.float32)


def embed_positions(rows, pos_fixed, P, step, blk_n):
    """the position of every row under the three modes of dec_embed_kernel"""
    r = np.arange(rows)
    if blk_n > 0:
        return pos_fixed + r % blk_n
    return np.full(rows, pos_fixed if pos_fixed >= 0 else P - 1 + step)


# ---------------------------------------------------------------- align post-processing
def _median_reflect(x, width):
    """median of `width` along the last axis with numpy `reflect` padding; identity when width // 2 == 0 or the axis is
    not longer than width // 2 (oracle.whisper._median_filter)"""
    pad = width // 2
    if pad == 0 or x.shape[-1] <= pad:
        return x
    xp = np.pad(x, [(0, 0)] * (x.ndim - 1) + [(pad, pad)], mode="reflect")
    win = np.lib.stride_tricks.sliding_window_view(xp, width, axis=-1)
    return np.sort(win, axis=-1)[..., pad]


def align_post_ref(probs, n_tok, nfr, width, mat):
    """fp64: per chunk b, over the first n_tok[b] token rows and nfr[b] frames of probs [B][n_sel][cap][T]: standardise
    over tokens (mean, population standard deviation per head and frame), median filter over frames, mean over heads.
    Returns a float64 copy of mat [B][cap][T] with exactly those entries replaced."""
    probs = np.asarray(probs, np.float64)
    out = np.array(mat, np.float64)
    for b in range(probs.shape[0]):
        n, F = int(n_tok[b]), int(nfr[b])
        w = probs[b, :, :n, :F]
        w = (w - w.mean(axis=-2, keepdims=True)) / w.std(axis=-2, keepdims=True)
        out[b, :n, :F] = _median_reflect(w, width).mean(axis=0)
    return out


def align_post_fp32(probs, n_tok, nfr, width, mat):
    """the same in float32 in the kernels' operation order: sequential sums over tokens for mean and variance,
    1 / sqrt(var), (p - mean) * rstd, median, sequential sum over heads, one division.  Used only to size the
    tolerance of the fp64 comparison (its distance from align_post_ref is what fp32 arithmetic costs on the input)."""
    f32 = np.float32
    probs = np.asarray(probs, f32)
    out = np.array(mat, f32)
    for b in range(probs.shape[0]):
        n, F = int(n_tok[b]), int(nfr[b])
        p = probs[b, :, :n, :F]
        mean = np.zeros((p.shape[0], F), f32)
        for i in range(n):
            mean = mean + p[:, i]
        mean = mean / f32(n)
        var = np.zeros_like(mean)
        for i in range(n):
            dlt = p[:, i] - mean
            var = var + dlt * dlt
        var = var / f32(n)
        rstd = f32(1.0) / np.sqrt(var)
        w = _median_reflect((p - mean[:, None]) * rstd[:, None], width)
        acc = np.zeros(w.shape[1:], f32)
        for hs in range(w.shape[0]):
            acc = acc + w[hs]
        out[b, :n, :F] = acc / f32(w.shape[0])
    return out
