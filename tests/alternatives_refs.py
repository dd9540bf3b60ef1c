"""Plain numpy references of the alternatives bookkeeping (the ALT instantiations of the rules kernel, dec_vocab.hip, and of the
beam update, dec_kernels.hip, and dec_alt_gather_kernel), on top of token_logprob_refs.beam_update_lp_ref, which stays the reference of
everything the existing contract covers.

  * top_n: the first n of a row's extraction — log-prob descending, id ascending, (0, -inf) once nothing is left;
  * beam_update_alt_ref: one beam-update step with the path of every hypothesis it records: fin_path[c][slot][q] for
    q < step = the source row's slot-table byte at P_c - 1 + q (the beam slot whose row produced token q), [step] = the
    source row's own beam index; nothing else of fin_path is touched.  ptab gives every chunk its own prompt length and
    budget P + budget - ptab[c] (a ragged run): chunks are independent, so it is the uniform reference chunk by chunk;
  * gather_ref: the compact [hyp][T + 1][n] arrays by numpy indexing."""
import numpy as np

from decode_state_refs import FIN_CAP
from token_logprob_refs import beam_update_lp_ref


def top_n(lp, n):
    """(ids, values) of the n most likely entries of a processed row: value descending, id ascending; dead tail (0, -inf)"""
    lp = np.asarray(lp)
    order = np.lexsort((np.arange(lp.shape[0]), -lp))[:n]
    ids, vals = order.astype(np.int32), lp[order].astype(np.float32)
    dead = ~np.isfinite(vals)
    ids[dead], vals[dead] = 0, -np.inf
    return ids, vals


_ROW_KEYS = ("hist2", "kvidx2", "cum2", "lphist2")            # [2][R][..]
_CHUNK_KEYS = ("done", "n_fin", "fin_tok", "fin_len", "fin_score", "fin_cum", "fin_lp")


def _chunk_state(state, c, K):
    s = {k: np.array(state[k][:, c * K:(c + 1) * K]) for k in _ROW_KEYS}
    s["cur_tok"] = np.array(state["cur_tok"][c * K:(c + 1) * K])
    s.update({k: np.array(state[k][c:c + 1]) for k in _CHUNK_KEYS})
    s["n_done"] = np.zeros(1, np.int32)
    return s


def beam_update_alt_ref(state, cand_val, cand_tok, cand_lp, fin_path, *, K, P, step, budget, max_fin, lp_pow, eot, ptab=None):
    """-> (new state as beam_update_lp_ref returns it, new fin_path [B][FIN_CAP][NT + 1] uint8)"""
    cand_val, cand_tok = np.asarray(cand_val, np.float32), np.asarray(cand_tok, np.int32)
    R, NT = state["hist2"].shape[1:]
    B, C = R // K, 2 * K
    kw = dict(K=K, step=step, max_fin=max_fin, lp_pow=lp_pow, eot=eot)
    if ptab is None:
        new = beam_update_lp_ref(state, cand_val, cand_tok, cand_lp, P=P, budget=budget, **kw)
    else:
        new = {k: np.array(v, copy=True) for k, v in state.items()}
        new["fin_score"] = new["fin_score"].astype(np.float64)
        for c in range(B):
            sl = slice(c * K, (c + 1) * K)
            one = beam_update_lp_ref(_chunk_state(state, c, K), cand_val[sl], cand_tok[sl], np.asarray(cand_lp)[sl],
                                     P=int(ptab[c]), budget=P + budget - int(ptab[c]), **kw)
            for k in _ROW_KEYS:
                new[k][:, sl] = one[k]
            new["cur_tok"][sl] = one["cur_tok"]
            for k in _CHUNK_KEYS:
                new[k][c:c + 1] = one[k]
            new["n_done"][0] += one["n_done"][0]
    path = np.array(fin_path, np.uint8, copy=True)
    cur = step & 1
    for c in range(B):
        if state["done"][c]:
            continue
        Pc = P if ptab is None else int(ptab[c])
        last_step = step + 1 >= (budget if ptab is None else P + budget - Pc)
        nsrc = 1 if step == 0 else K
        flat_v = cand_val[c * K:c * K + nsrc].reshape(-1)
        flat_t = cand_tok[c * K:c * K + nsrc].reshape(-1)
        order = [int(i) for i in np.argsort(-flat_v, kind="stable") if flat_v[i] != -np.inf][:C]
        nf = int(state["n_fin"][c])
        for slot in range(min(K, len(order))):
            j = order[slot]
            if (flat_t[j] == eot or last_step) and nf < FIN_CAP:
                src = c * K + j // C
                path[c, nf, :step] = state["kvidx2"][cur, src, Pc - 1:Pc - 1 + step]
                path[c, nf, step] = j // C
                nf += 1
        assert nf == int(new["n_fin"][c])
    return new, path


def gather_ref(alt_tok, alt_lp, fin_path, hyps, K, T):
    """alt_tok / alt_lp [steps][R][n], hyps [(chunk, slot, len, end | -1)] -> out_tok, out_lp [n_hyp][T + 1][n]"""
    n = alt_tok.shape[2]
    out_t = np.full((len(hyps), T + 1, n), -1, np.int32)
    out_l = np.zeros((len(hyps), T + 1, n), np.float32)
    for i, (c, f, ln, end) in enumerate(hyps):
        for t in range(ln):
            out_t[i, t], out_l[i, t] = alt_tok[t, c * K + fin_path[c, f, t]], alt_lp[t, c * K + fin_path[c, f, t]]
        if end >= 0:
            out_t[i, T], out_l[i, T] = alt_tok[end, c * K + fin_path[c, f, end]], alt_lp[end, c * K + fin_path[c, f, end]]
    return out_t, out_l


def check_alternatives(tokens, token_logprobs, alts, greedy=False):
    """the exact identities between a hypothesis' chosen tokens and the alternatives of their positions: every list sorted by
    (log-prob descending, id ascending); a chosen token that is in its list has its recorded log-prob there, bit for bit;
    one that is not lies at or below the list's last entry; greedy: entry 0 IS the chosen token.  Returns how many chosen
    tokens were found in their lists."""
    assert len(tokens) == len(token_logprobs) == len(alts)
    found = 0
    for t, (tok, lp, alt) in enumerate(zip(tokens, token_logprobs, alts)):
        keys = [(-v, i) for i, v in alt]
        assert keys == sorted(keys), (t, alt)
        live = [(i, v) for i, v in alt if v != -np.inf]
        assert all(i == 0 for i, v in alt if v == -np.inf) and alt[:len(live)] == live, (t, alt)
        assert len({i for i, _ in live}) == len(live), (t, alt)
        hit = [v for i, v in live if i == tok]
        if hit:
            assert np.float32(hit[0]).view(np.uint32) == np.float32(lp).view(np.uint32), (t, tok, hit, lp)
            found += 1
        else:
            assert lp <= alt[-1][1], (t, tok, lp, alt)
        if greedy:
            assert alt[0][0] == tok and np.float32(alt[0][1]).view(np.uint32) == np.float32(lp).view(np.uint32), (t, alt, tok, lp)
    return found
