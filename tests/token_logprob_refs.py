"""Plain numpy reference of the per-token log-prob bookkeeping of the beam update (dec_kernels.hip K19/K20 with cand_lp /
lphist2 / fin_lp), on top of decode_state_refs.beam_update_ref, which stays the reference of everything the existing
contract covers (tokens, slot table, cum, finished hypotheses, done).

Contract of the new arrays, per chunk that is not done on entry (the values are copied, never computed):
  * a candidate carries its cand_lp through merge and walk exactly as it carries its token;
  * a finished hypothesis, recorded while fewer than FIN_CAP are held, gets fin_lp[c][n][:step] = lphist2[cur][parent][:step];
    a real token (last step) puts its cand_lp at [step] and 0.0 into the end slot [NT], an <eot> puts its cand_lp into the
    end slot;
  * when the chunk goes on, row k's lphist2[nxt][k][:step] = lphist2[cur][parent][:step] and [step] = the cand_lp of the
    chosen candidate; dead beams copy live beam 0's;
  * a chunk that finishes, or was done on entry, rewrites no row state."""
import numpy as np

from decode_state_refs import FIN_CAP, beam_state, beam_update_ref


def lp_state(B, K, NT, step, P, hist, lphist, kvidx, cum, sentinel_i, sentinel_f, fin_lp=None, **kw):
    """decode_state_refs.beam_state plus lphist2 [2][R][NT] (lphist [R][step] in parity half step & 1, sentinel_f
    elsewhere) and fin_lp [B][FIN_CAP][NT + 1] (as it stands, or all sentinel_f)"""
    st = beam_state(B, K, NT, step, P, hist, kvidx, cum, sentinel_i, sentinel_f, **kw)
    R = B * K
    st["lphist2"] = np.full((2, R, NT), sentinel_f, np.float32)
    if step:
        st["lphist2"][step & 1, :, :step] = np.asarray(lphist, np.float32).reshape(R, step)
    st["fin_lp"] = np.full((B, FIN_CAP, NT + 1), sentinel_f, np.float32) if fin_lp is None else np.array(fin_lp, np.float32)
    return st


def beam_update_lp_ref(state, cand_val, cand_tok, cand_lp, *, K, P, step, budget, max_fin, lp_pow, eot):
    """One beam-update step on `state` (lp_state's layout; not modified) -> the new state, log-prob arrays included."""
    base = {k: v for k, v in state.items() if k not in ("lphist2", "fin_lp")}
    s = beam_update_ref(base, cand_val, cand_tok, K=K, P=P, step=step, budget=budget, max_fin=max_fin, lp_pow=lp_pow,
                        eot=eot)
    s["lphist2"] = np.array(state["lphist2"], np.float32, copy=True)
    s["fin_lp"] = np.array(state["fin_lp"], np.float32, copy=True)
    cand_val = np.asarray(cand_val, np.float32)
    cand_tok = np.asarray(cand_tok, np.int32)
    cand_lp = np.asarray(cand_lp, np.float32)
    R, NT = state["hist2"].shape[1:]
    B, C = R // K, 2 * K
    cur, nxt = step & 1, (step & 1) ^ 1
    last_step = step + 1 >= budget
    for c in range(B):
        if state["done"][c]:
            continue
        nsrc = 1 if step == 0 else K
        flat_v = cand_val[c * K:c * K + nsrc].reshape(-1)
        flat_t = cand_tok[c * K:c * K + nsrc].reshape(-1)
        flat_l = cand_lp[c * K:c * K + nsrc].reshape(-1)
        order = [int(i) for i in np.argsort(-flat_v, kind="stable") if flat_v[i] != -np.inf][:C]
        nf = int(state["n_fin"][c])
        sec, live = K, []
        for slot in range(min(K, len(order))):
            j = order[slot]
            if flat_t[j] == eot or last_step:
                if nf < FIN_CAP:
                    s["fin_lp"][c, nf, :step] = state["lphist2"][cur, c * K + j // C, :step]
                    if flat_t[j] != eot:
                        s["fin_lp"][c, nf, step] = flat_l[j]
                        s["fin_lp"][c, nf, NT] = np.float32(0.0)
                    else:
                        s["fin_lp"][c, nf, NT] = flat_l[j]
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
            live.append((j // C, flat_l[j]))
        assert nf == int(s["n_fin"][c])
        if s["done"][c]:
            continue
        assert live
        while len(live) < K:
            live.append(live[0])
        for k, (par, lp) in enumerate(live):
            s["lphist2"][nxt, c * K + k, :step] = state["lphist2"][cur, c * K + par, :step]
            s["lphist2"][nxt, c * K + k, step] = lp
    return s
