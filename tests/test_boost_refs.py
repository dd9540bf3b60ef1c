"""Phrase boosting on the host (no GPU): the numpy restatement (tests/boost_refs.py) against hand-written cases, the
table fw_boost_create compiles — walked in plain C++ by fw_test_boost_rows_host — against the restatement on seeded random
lists and histories, bit for bit, and every limit of fw_boost_create."""
import numpy as np
import pytest

from faster_whisper_amd import _lib

import boost_refs as br
from boost_refs import MAX_LEN, MAX_PHRASES, MAX_TOKENS


# ---- the restatement against hand-written cases ----
def test_repeated_phrase_boosts_once():
    a = 7
    assert br.boost_of_row([[a, a, a]], [1.5], [a, a]) == {a: np.float32(1.5)}      # k = 0, 1, 2 all match: a max, not 4.5
    lg = np.zeros((1, 10), dtype=np.float32)
    out = br.boost_rows(lg, [[a, a, a]], [1.5], [[a, a]])
    assert out[0, a] == np.float32(1.5) and np.count_nonzero(out) == 1


def test_mixed_signs_on_one_id_take_the_maximum():
    assert br.boost_of_row([[3], [3]], [2.0, -3.0], []) == {3: np.float32(2.0)}
    assert br.boost_of_row([[3], [3]], [-3.0, 2.0], [5, 5]) == {3: np.float32(2.0)}
    assert br.boost_of_row([[3]], [-3.0], []) == {3: np.float32(-3.0)}              # alone, a negative boost counts


def test_empty_history_boosts_first_tokens_only():
    assert br.boost_of_row([[1, 2, 3], [4]], [1.0, 2.0], []) == {1: np.float32(1.0), 4: np.float32(2.0)}


def test_history_shorter_than_the_phrase():
    p = [1, 2, 3, 4, 5]
    assert br.boost_of_row([p], [1.0], [1, 2]) == {1: np.float32(1.0), 3: np.float32(1.0)}
    assert br.boost_of_row([p], [1.0], [2]) == {1: np.float32(1.0)}                 # (k = 1 needs h[-1] == 1)
    assert br.boost_of_row([p], [1.0], [9, 1, 2, 3, 4]) == {1: np.float32(1.0), 5: np.float32(1.0)}
    # a prefix that differs only in its EARLIEST token does not match
    assert br.boost_of_row([p], [1.0], [8, 2, 3, 4]) == {1: np.float32(1.0)}


def test_one_add_and_untouched_ids():
    lg = np.array([[0.1, -np.inf, 3.0, 1e30]], dtype=np.float32)
    out = br.boost_rows(lg, [[1], [2], [3]], [5.0, 0.25, 1e30], [[]])
    assert br.bits(out)[0, 0] == br.bits(lg)[0, 0]
    assert out[0, 1] == -np.inf and out[0, 2] == np.float32(3.25) and out[0, 3] == np.float32(np.float32(1e30) + np.float32(1e30))


# ---- the compiled table, walked on the host, against the restatement ----
def _random_case(rng, V, n_phrases, max_len, alphabet):
    phrases = [list(rng.choice(alphabet, size=int(rng.integers(1, max_len + 1)))) for _ in range(n_phrases)]
    boosts = rng.uniform(-4, 8, size=n_phrases).astype(np.float32)
    hists = [list(rng.choice(alphabet, size=int(n))) for n in rng.integers(0, 40, size=6)]
    # some histories END with the prefix of a phrase, so that long matches occur too
    for r in range(0, len(hists), 2):
        p = phrases[int(rng.integers(n_phrases))]
        hists[r] = hists[r] + p[:int(rng.integers(0, len(p)))]
    logits = rng.standard_normal((len(hists), V)).astype(np.float32) * 5
    return phrases, boosts, hists, logits


@pytest.mark.parametrize("seed,V,n_phrases,max_len,n_alpha", [(0, 50, 8, 4, 3), (1, 1913, 64, 32, 5), (2, 1913, 300, 6, 40),
                                                             (3, 51865, 1024, 4, 2000)])
def test_host_walk_matches_the_restatement(seed, V, n_phrases, max_len, n_alpha):
    rng = np.random.default_rng(seed)
    alphabet = rng.choice(V, size=n_alpha, replace=False)
    phrases, boosts, hists, logits = _random_case(rng, V, n_phrases, max_len, alphabet)
    want = br.boost_rows(logits, phrases, boosts, hists)
    got = br.rows_host(logits, hists, br.Boost(V, phrases, boosts))
    assert np.array_equal(br.bits(got), br.bits(want))
    assert np.any(br.bits(got) != br.bits(logits))          # (something was boosted)


def test_host_walk_hand_cases():
    V, a = 20, 4
    lg = np.linspace(-1, 1, 3 * V, dtype=np.float32).reshape(3, V)
    hists = [[a, a], [], [1, 2]]
    phrases, boosts = [[a, a, a], [a], [1, 2, 19], [0]], [1.5, -3.0, 2.0, 0.5]
    got = br.rows_host(lg, hists, br.Boost(V, phrases, boosts))
    want = br.boost_rows(lg, phrases, boosts, hists)
    assert np.array_equal(br.bits(got), br.bits(want))
    assert got[0, a] == np.float32(lg[0, a] + np.float32(1.5)) and got[2, 19] == np.float32(lg[2, 19] + np.float32(2.0))


def test_empty_list_touches_nothing():
    V = 100
    lg = np.ones((2, V), dtype=np.float32)
    out = br.rows_host(lg, [[1], []], br.Boost(V, [], []))
    assert np.array_equal(br.bits(out), br.bits(lg))


# ---- the limits ----
def _rc(n_vocab, phrases, boosts):
    rc, h = br.create_rc(n_vocab, phrases, boosts)
    if h:
        _lib.load().fw_boost_free(h)
    assert (rc == _lib.FW_OK) == bool(h)
    return rc


def test_limits_accepted():
    assert _rc(10, [], []) == _lib.FW_OK                                              # an empty list
    assert _rc(10, [[1]] * MAX_PHRASES, [1.0] * MAX_PHRASES) == _lib.FW_OK
    assert _rc(10, [[2] * MAX_LEN], [1.0]) == _lib.FW_OK
    assert _rc(10, [[3] * MAX_LEN] * (MAX_TOKENS // MAX_LEN), [1.0] * (MAX_TOKENS // MAX_LEN)) == _lib.FW_OK
    assert _rc(10, [[0], [9]], [-1e30, 3.4e38]) == _lib.FW_OK                         # ids 0 and n_vocab - 1, any finite boost


def test_limits_refused():
    E = _lib.FW_EINVAL
    assert _rc(10, [[1]] * (MAX_PHRASES + 1), [1.0] * (MAX_PHRASES + 1)) == E
    assert _rc(10, [[2] * (MAX_LEN + 1)], [1.0]) == E
    n = MAX_TOKENS // MAX_LEN
    assert _rc(10, [[3] * MAX_LEN] * n + [[3]], [1.0] * (n + 1)) == E                 # 4097 tokens
    assert _rc(10, [[1], []], [1.0, 1.0]) == E                                        # L_j = 0
    assert _rc(10, [[10]], [1.0]) == E                                                # an id equal to n_vocab
    assert _rc(10, [[-1]], [1.0]) == E
    for bad in (np.nan, np.inf, -np.inf):
        assert _rc(10, [[1]], [bad]) == E
    assert _rc(0, [], []) == E
    with pytest.raises(ValueError):
        br.Boost(10, [[10]], [1.0])
