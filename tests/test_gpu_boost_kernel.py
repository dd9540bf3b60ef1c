"""dec_boost_kernel alone, through fw_test_boost_rows (include/fwamd_test.h), against the numpy restatement of phrase
boosting (tests/boost_refs.py) on the micro vocabulary (V = 1913, text context 448): the WHOLE logits of every launch are
compared as uint32 — the boosted ids carry one fp32 add, every other value the caller's bits.  Both row forms: 0 = the
decode step (parity half of hist2, one n for all rows, done chunks skipped), 1 = scoring (a ScoreRow per row, ragged
histories, rows without a target skipped)."""
import numpy as np
import pytest

import boost_refs as br

pytestmark = pytest.mark.gpu

V = 1913
FORMS = [0, 1]


@pytest.fixture(scope="module")
def env():
    from faster_whisper_amd import Whisper, get_config, synthetic_weights
    cfg = get_config("micro")
    assert cfg.n_vocab == V
    model = Whisper("synthetic:boost", device="cuda", files={"config": cfg, "weights": synthetic_weights(cfg, seed=5)},
                    max_batch_size=2, max_beam_size=5)
    return cfg, model, model._replicas[0].handle


def _logits(rows, seed):
    return (np.random.default_rng(seed).standard_normal((rows, V)) * 4).astype(np.float32)


def _check(handle, logits, phrases, boosts, hists, form, K=1, done=None, skipped=()):
    want = br.boost_rows(logits, phrases, boosts, hists)
    for r in skipped:
        want[r] = logits[r]
    got = br.rows_gpu(handle, logits, hists, br.Boost(V, phrases, boosts), form, K=K, done=done)
    assert np.array_equal(br.bits(got), br.bits(want)), np.argwhere(br.bits(got) != br.bits(want))[:8]
    return got


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", [0, 1, 31, 447])
def test_history_lengths_and_phrase_lengths(env, form, n):
    """phrases of 1, 2 and 32 tokens, target ids 0 and V - 1, against histories of n tokens: row 0 ends with the longest
    prefix of the 32-token phrase that fits, row 1 with one that differs only in its EARLIEST token, row 2 is random"""
    _, _, handle = env
    rng = np.random.default_rng(10 + n)
    long = [int(t) for t in rng.choice(np.arange(8, 400), size=32, replace=False)]
    long[-1] = V - 1
    phrases = [[0], [7, V - 1], long, [long[0], 0]]
    boosts = [1.25, -2.5, 3.0, 0.5]
    rows = []
    k = min(n, 31)
    base = [int(t) for t in rng.integers(8, 400, size=n)]
    rows.append((base[:n - k] + long[:k]) if k else base)
    broken = list(rows[0])
    if k:
        broken[n - k] = long[0] % 399 + 1                         # any other id
    rows.append(broken)
    rows.append(base)
    lg = _logits(3, n)
    got = _check(handle, lg, phrases, boosts, rows, form)
    assert got[0, 0] != lg[0, 0]                                  # the one-token phrase: every row, every n
    if 0 < k < 32:
        assert got[0, long[k]] == np.float32(lg[0, long[k]] + np.float32(3.0)) and got[1, long[k]] == lg[1, long[k]]


@pytest.mark.parametrize("form", FORMS)
def test_more_target_ids_than_threads_and_the_full_table(env, form):
    """1024 phrases of 4 tokens = the full 4096 tokens; 600 distinct target ids (more than the workgroup's 256 threads),
    shared first tokens with mixed signs (the maximum counts), and histories that end inside some of the phrases"""
    _, _, handle = env
    rng = np.random.default_rng(3)
    ids = rng.choice(V, size=600, replace=False)
    phrases = [[int(t) for t in rng.choice(ids, size=4)] for _ in range(br.MAX_PHRASES)]
    for j in range(600):
        phrases[j][j % 4] = int(ids[j])                            # every one of the 600 ids is a target
    boosts = rng.uniform(-3, 6, size=br.MAX_PHRASES).astype(np.float32)
    assert sum(len(p) for p in phrases) == br.MAX_TOKENS and len({t for p in phrases for t in p}) > 256
    hists = []
    for r in range(4):
        h = [int(t) for t in rng.choice(ids, size=20)] + phrases[int(rng.integers(br.MAX_PHRASES))][:1 + r % 3]
        hists.append(h[-21:])                                     # (form 0 takes one n)
    _check(handle, _logits(4, 4), phrases, boosts, hists, form)


@pytest.mark.parametrize("form", FORMS)
def test_minus_infinity_stays_and_empty_list_touches_nothing(env, form):
    _, _, handle = env
    lg = _logits(2, 5)
    lg[0, 9] = -np.inf
    got = _check(handle, lg, [[9], [10]], [1e4, 1e4], [[3], [3]], form)
    assert got[0, 9] == -np.inf and got[1, 9] == np.float32(lg[1, 9] + np.float32(1e4))
    got = br.rows_gpu(handle, lg, [[3], [3]], br.Boost(V, [], []), form)
    assert np.array_equal(br.bits(got), br.bits(lg))


def test_repeated_phrase_and_mixed_signs(env):
    _, _, handle = env
    a = 33
    lg = _logits(2, 6)
    for form in FORMS:
        got = _check(handle, lg, [[a, a, a], [50], [50]], [1.5, 2.0, -3.0], [[a, a], [a, a]], form)
        assert got[0, a] == np.float32(lg[0, a] + np.float32(1.5)) and got[0, 50] == np.float32(lg[0, 50] + np.float32(2.0))


def test_step_form_skips_done_chunks(env):
    """R = 10, K = 5: the rows of the chunk marked done keep the caller's bits, the other chunk's rows are boosted with
    their own histories (the beams of a chunk differ)"""
    _, _, handle = env
    rng = np.random.default_rng(7)
    phrases, boosts = [[20, 21, 22], [21], [0]], [2.0, -1.0, 0.75]
    hists = [[int(t) for t in rng.integers(19, 23, size=5)] for _ in range(10)]
    hists[1][-1] = 20
    hists[6][-2:] = [20, 21]
    lg = _logits(10, 8)
    for done in ([0, 1], [1, 0]):
        skipped = [r for r in range(10) if done[r // 5]]
        got = _check(handle, lg, phrases, boosts, hists, 0, K=5, done=done, skipped=skipped)
        assert all(np.array_equal(br.bits(got[r]), br.bits(lg[r])) for r in skipped)
        assert all(got[r, 0] != lg[r, 0] for r in range(10) if r not in skipped)


def test_score_form_ragged_histories_and_a_row_without_target(env):
    _, _, handle = env
    phrases, boosts = [[20, 21, 22], [21, 5], [V - 1]], [2.0, 4.0, -0.5]
    hists = [[], [20], [9, 20, 21], [21] * 40, [20, 21], list(range(100, 547))]
    lg = _logits(len(hists), 9)
    done = [0, 0, 0, 0, 1, 0]
    got = _check(handle, lg, phrases, boosts, hists, 1, done=done, skipped=[4])
    assert np.array_equal(br.bits(got[4]), br.bits(lg[4]))
    assert got[2, 22] == np.float32(lg[2, 22] + np.float32(2.0)) and got[3, 5] == np.float32(lg[3, 5] + np.float32(4.0))


def test_hook_refuses_wrong_tests(env):
    """FW_EINVAL before anything is launched, the logits left alone"""
    cfg, _, handle = env
    lg = _logits(2, 11)
    good = br.Boost(V, [[1, 2]], [1.0])
    cases = [
        dict(hists=[[1], [1, 2]], boost=good, form=0),                     # form 0 with two different n
        dict(hists=[[1], [2]], boost=good, form=2),                        # no such form
        dict(hists=[[1], [2]], boost=good, form=0, K=3),                   # rows % K
        dict(hists=[[1], [2]], boost=good, form=1, K=2),                   # form 1 takes K = 1
        dict(hists=[[1], [V]], boost=good, form=1),                        # a history id outside the vocabulary
        dict(hists=[[1] * cfg.n_text_ctx] * 2, boost=good, form=1),        # a history as long as the text context
        dict(hists=[[1], [2]], boost=good, form=0, done=[2, 0]),              # done is 0 / 1
        dict(hists=[[1], [2]], boost=br.Boost(V + 1, [[1]], [1.0]), form=0),   # a list for another vocabulary
    ]
    for c in cases:
        with pytest.raises(ValueError):
            br.rows_gpu(handle, lg, c["hists"], c["boost"], c["form"], K=c.get("K", 1), done=c.get("done"))
