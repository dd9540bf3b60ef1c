"""dec_constrain_kernel alone, through fw_test_constrain_rows (include/fwamd_test.h), against the numpy restatement of
constrained decoding (tests/constrain_refs.py).  The hook takes the vocabulary geometry from the test, so the row stride V
is chosen: V in {203 .. 206} with five rows puts a row start at every 16-byte residue, with an even and an odd row each
where the residue recurs.  The WHOLE logits of every launch are compared as uint32: an allowed id carries the caller's
bits (-inf and 3e38 among them), every other one -inf, and a skipped row — a done chunk's, a score row without target —
is untouched, also by the peeled head and tail stores of the rows beside it.  Both row forms: 0 = the decode step (parity
half of hist2, one n for all rows), 1 = scoring (a ScoreRow per row, ragged histories)."""
import numpy as np
import pytest

import constrain_refs as cr

pytestmark = pytest.mark.gpu

FORMS = [0, 1]
VS = [203, 204, 205, 206]
EOT, TSB = 150, 160                        # inside every V of VS
L = 6
LONG = list(range(100, 132))


@pytest.fixture(scope="module")
def handle():
    from faster_whisper_amd import Whisper, get_config, synthetic_weights
    cfg = get_config("micro")
    model = Whisper("synthetic:constrain", device="cuda", files={"config": cfg, "weights": synthetic_weights(cfg, seed=5)},
                    max_batch_size=2, max_beam_size=5)
    yield model._replicas[0].handle
    del model


def _logits(rows, V, seed):
    """random, with -inf and large magnitudes of both signs on ids the lists allow and on ids they do not"""
    lg = (np.random.default_rng(seed).standard_normal((rows, V)) * 4).astype(np.float32)
    for r in range(rows):
        lg[r, [1, 11, (7 * r + 3) % V]] = [-np.inf, np.float32(3e38), np.float32(-3e38)]
        lg[r, V - 1] = np.float32(1e30)
    return lg


def _check(handle, lg, phrases, hists, form, with_ts, eot=EOT, tsb=TSB, K=1, done=None, skipped=()):
    want = cr.constrain_rows(lg, phrases, hists, eot, tsb, with_ts)
    for r in skipped:
        want[r] = lg[r]
    got = cr.rows_gpu(handle, lg, hists, cr.Constraint(lg.shape[1], phrases), eot, tsb, with_ts, form, K=K, done=done)
    assert np.array_equal(cr.bits(got), cr.bits(want)), np.argwhere(cr.bits(got) != cr.bits(want))[:8]
    return got


PHRASES = [[11, 12, 13, 14, 15, 16], [11, 12, 99], [11], [1, 2], [1, 2], LONG, [149]]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("with_ts", [False, True])
@pytest.mark.parametrize("V", VS)
def test_every_row_alignment_and_text_lengths(handle, V, with_ts, form):
    """five rows per launch; text lengths 0, 1, L - 1, L, L + 1 and 33 of a phrase of L = 6 and one of 32"""
    p6 = PHRASES[0]
    for n, rows in [(0, [[]] * 5),
                    (1, [[11], [1], [12], [100], [149]]),
                    (L - 1, [p6[:5], p6[:4] + [99], [11, 12, 99, 1, 2], LONG[:5], [11] * 5]),
                    (L, [p6, p6[:5] + [17], LONG[:6], [1, 2, 1, 2, 1, 2], [11, 12, 13, 14, 15, 99]]),
                    (L + 1, [p6 + [16], p6 + [11], LONG[:7], [11] + p6, LONG[1:8]]),
                    (31, [LONG[:31], LONG[:30] + [1], LONG[1:32], [11] * 31, LONG[:31]]),
                    (32, [LONG, LONG[:31] + [1], LONG, [1] * 32, LONG[::-1]]),
                    (33, [LONG + [11], LONG + [LONG[0]], [11] * 33, LONG[:1] * 33, LONG + [132]])]:
        got = _check(handle, _logits(5, V, n), PHRASES, rows, form, with_ts)
        if n == 0:
            assert got[0, 11] == np.float32(3e38) and got[0, 1] == -np.inf and got[0, 100] != -np.inf
        if n == 32:
            assert np.flatnonzero(got[0, :TSB] != -np.inf).tolist() == [EOT]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("with_ts", [False, True])
def test_timestamps_interleaved(handle, form, with_ts):
    """timestamp ids anywhere in the history do not count: the rows below have the text [11, 12] behind 5 history ids"""
    t = TSB + 3
    hists = [[t, 11, t, t + 1, 12], [11, 12, t, t, t], [t, t, t, 11, 12], [t, 11, t + 40, 12, t + 40], [t, t, t, t, t]]
    got = _check(handle, _logits(5, 205, 3), PHRASES, hists, form, with_ts)
    for r in range(4):
        assert sorted(np.flatnonzero(got[r, :TSB] != -np.inf).tolist()) == [13, 99]
    assert np.all(got[:, TSB:] != -np.inf) if with_ts else np.all(got[:, TSB:] == -np.inf)
    # more than a workgroup's worth of history in front of the text: 300 timestamps, then [11, 12]
    got = _check(handle, _logits(2, 206, 4), PHRASES, [[t] * 300 + [11, 12], [11] + [t] * 300 + [12]], form, with_ts)
    assert sorted(np.flatnonzero(got[1, :TSB] != -np.inf).tolist()) == [13, 99]


@pytest.mark.parametrize("V", VS)
def test_step_form_skips_done_chunks_and_does_not_overrun_them(handle, V):
    """R = 10, K = 5: the rows of the done chunk keep every bit — the rows in front of and behind them are written up to
    their last and from their first id, whatever the alignment"""
    hists = [[11, 12], [11, 12], [1, 2], [11, 13], [TSB, 11], [11, 12], [100, 101], [1, 2], [TSB + 1, TSB + 1], [11, 99]]
    lg = _logits(10, V, 8)
    for done in ([0, 1], [1, 0]):
        skipped = [r for r in range(10) if done[r // 5]]
        got = _check(handle, lg, PHRASES, hists, 0, False, K=5, done=done, skipped=skipped)
        assert all(np.array_equal(cr.bits(got[r]), cr.bits(lg[r])) for r in skipped)
        assert all(got[r, V - 1] == -np.inf and got[r, 0] == -np.inf for r in range(10) if r not in skipped)


@pytest.mark.parametrize("V", VS)
def test_score_form_rows_without_target_are_unchanged(handle, V):
    hists = [[], [11], [11, 12, 13], [TSB] * 40, [11, 12], LONG + [1], [1]]
    lg = _logits(len(hists), V, 9)
    done = [0, 1, 0, 0, 1, 0, 1]
    got = _check(handle, lg, PHRASES, hists, 1, True, done=done, skipped=[1, 4, 6])
    for r in (1, 4, 6):
        assert np.array_equal(cr.bits(got[r]), cr.bits(lg[r]))
    assert np.all(got[5, :TSB] == -np.inf)


@pytest.mark.parametrize("form", FORMS)
def test_a_root_of_300_children_and_the_full_table(handle, form):
    """more first ids than the workgroup has threads; then 1024 phrases of 4 tokens = the full 4096 tokens"""
    V, eot, tsb = 1913, 400, 412
    rng = np.random.default_rng(3)
    firsts = [int(t) for t in rng.choice(eot, size=300, replace=False)]
    phrases = [[f] for f in firsts[:100]] + [[f, (f * 7) % eot] for f in firsts[100:]]
    lg = (rng.standard_normal((4, V)) * 4).astype(np.float32)
    got = _check(handle, lg, phrases, [[], [], [], []], form, False, eot=eot, tsb=tsb)
    assert np.count_nonzero(got[0] != -np.inf) == 300
    hists = [[firsts[0]], [firsts[150]], [firsts[299]], [next(i for i in range(eot) if i not in firsts)]]
    _check(handle, lg, phrases, hists, form, True, eot=eot, tsb=tsb)
    phrases = [[int(t) for t in rng.integers(0, 40, size=4)] for _ in range(cr.MAX_PHRASES)]
    assert sum(len(p) for p in phrases) == cr.MAX_TOKENS
    hists = [phrases[5][:3], phrases[700][:3], phrases[1023][:3], [39, 39, 39]]          # (form 0 takes one n)
    _check(handle, lg, phrases, hists, form, True, eot=eot, tsb=tsb)
    hists = [phrases[1023], phrases[0], [39] * 4, phrases[5][:3] + [tsb]]
    _check(handle, lg, phrases, hists, form, True, eot=eot, tsb=tsb)
    _check(handle, lg, phrases, [[], [], [], []], form, False, eot=eot, tsb=tsb)


@pytest.mark.parametrize("form", FORMS)
def test_the_real_stride(handle, form):
    """V = 51866 (large-v3), three rows: r * 51866 mod 4 = 0, 2, 0 — row starts on 16, 8 and 16 bytes"""
    V, eot, tsb = 51866, 50257, 50365
    rng = np.random.default_rng(11)
    phrases = [[int(t) for t in rng.integers(0, 50000, size=int(rng.integers(1, 8)))] for _ in range(40)]
    phrases += [[50256], [0], [50000, 50255]]
    lg = (rng.standard_normal((3, V)) * 4).astype(np.float32)
    lg[:, [0, 50256, V - 1]] = np.float32(3e38)
    for with_ts in (False, True):
        got = _check(handle, lg, phrases, [[], [], []], form, with_ts, eot=eot, tsb=tsb)
        assert got[1, 0] == np.float32(3e38) and got[2, 50256] == np.float32(3e38)
        _check(handle, lg, phrases, [[tsb, phrases[3][0]], [tsb + 7] + phrases[40], [50000, tsb + 1]], form, with_ts, eot=eot, tsb=tsb)


def test_hook_refuses_wrong_tests(handle):
    """FW_EINVAL before anything is launched"""
    lg = _logits(2, 204, 11)
    good = cr.Constraint(204, [[1, 2]])
    cases = [
        dict(hists=[[1], [1, 2]], form=0),                                 # form 0 with two different n
        dict(hists=[[1], [2]], form=2),                                    # no such form
        dict(hists=[[1], [2]], form=0, K=3),                               # rows % K
        dict(hists=[[1], [2]], form=1, K=2),                               # form 1 takes K = 1
        dict(hists=[[1], [204]], form=1),                                  # a history id outside the vocabulary
        dict(hists=[[1] * 448] * 2, form=1),                               # a history as long as the text context
        dict(hists=[[1], [2]], form=0, done=[2, 0]),                       # done is 0 / 1
        dict(hists=[[1], [2]], form=0, c=cr.Constraint(205, [[1]])),       # a list for another vocabulary
        dict(hists=[[1], [2]], form=0, eot=TSB),                           # <eot> not below the first timestamp
        dict(hists=[[1], [2]], form=0, tsb=205),                           # first timestamp beyond the vocabulary
        dict(hists=[[1], [2]], form=0, with_ts=2),
    ]
    for c in cases:
        with pytest.raises(ValueError):
            cr.rows_gpu(handle, lg, c["hists"], c.get("c", good), c.get("eot", EOT), c.get("tsb", TSB), c.get("with_ts", 1),
                        c["form"], K=c.get("K", 1), done=c.get("done"))
