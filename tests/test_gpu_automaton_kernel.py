"""dec_automaton_kernel alone, through fw_test_automaton_rows, against the plain walk of tests/automaton_refs.py: the WHOLE
logits of every launch as uint32, both row forms (0 = decode step, 1 = scoring), all three stagings (the product's rule,
L2, LDS).  V = 67 with five rows puts a row start at every 16-byte residue; V = 51866 is large-v3's stride."""
import numpy as np
import pytest

import automaton_refs as ar

pytestmark = pytest.mark.gpu

GEOMETRY = {67: (50, 56), 51866: (50257, 50365)}      # V -> (<eot>, first timestamp)
NT = 448                                               # the micro model's text context: histories hold up to NT - 1 ids


@pytest.fixture(scope="module")
def handle():
    from faster_whisper_amd import Whisper, get_config, synthetic_weights
    cfg = get_config("micro")
    model = Whisper("synthetic:automaton", device="cuda", files={"config": cfg, "weights": synthetic_weights(cfg, seed=5)},
                    max_batch_size=2, max_beam_size=5)
    yield model._replicas[0].handle
    del model


def _loop2(eot, tsb):
    """0 -5-> 1 -9-> 0, state 1 accepting; the longest walk, a last step that leaves, timestamps anywhere, the empty history"""
    csr = ([0, 1, 2], [5, 9], [1, 0], [0, 1])
    walk = ([5, 9] * NT)[:NT - 1]
    with_ts = [t for pair in zip(walk, [tsb + 3] * NT) for t in pair][:NT - 1]
    return csr, [[walk, walk[:-1] + [9], with_ts, [5] + [tsb] * (NT - 2), [tsb + 1] * (NT - 1)],
                 [[]] * 5, [[5, 9, 5], [5, tsb, 9], [9, 5, 9], [5, 5, 5], [tsb, tsb, 5]]]


def _star(degree):
    def build(eot, tsb):
        """state 0 with `degree` children on ids 3 i + 1 (more than 64, than 256 threads, than one round of 4096)"""
        toks = [3 * i + 1 for i in range(degree)]
        csr = ([0, degree, degree, degree + 1], toks + [7], [1 + i % 2 for i in range(degree)] + [1], [0, 1, 0])
        ones = [[toks[0]], [toks[-1]], [toks[degree // 2]], [toks[63]], [toks[64]], [toks[-1] + 2], [0], [toks[100] + 1]]
        return csr, [ones, [[]] * 4, [[toks[1], 7], [toks[0], 7], [tsb, toks[65]], [toks[3], toks[3]]]]
    return build


def _limits(eot, tsb):
    """FW_AUTOMATON_MAX_STATES states, FW_AUTOMATON_MAX_EDGES edges: state s goes to s + 1 on s % 40 and to 7 s + 3 on 40 + s % 5"""
    S = 4096
    csr = ([2 * s for s in range(S + 1)], [t for s in range(S) for t in (s % 40, 40 + s % 5)],
           [t for s in range(S) for t in ((s + 1) % S, (7 * s + 3) % S)], [int(s % 3 == 0) for s in range(S)])
    rng = np.random.default_rng(2)

    def walk(n):
        s, out = 0, []
        for pick in rng.integers(0, 2, size=n):
            out.append(csr[1][2 * s + pick])
            s = csr[2][2 * s + pick]
        return out
    long = [walk(NT - 1), walk(NT - 1), walk(200) + [tsb + 9] * (NT - 201), walk(300)[:-1] + [45] + walk(NT - 301), walk(NT - 1)]
    return csr, [long, [walk(17), walk(17), walk(16) + [46], [tsb] * 17, walk(17)]]


CASES = {"loop2": (_loop2, (67, 51866)), "limits": (_limits, (67, 51866)), "star300": (_star(300), (51866,)),
         "star5000": (_star(5000), (51866,))}


def _logits(rows, V, seed):
    lg = (np.random.default_rng(seed).standard_normal((rows, V)) * 4).astype(np.float32)
    lg[:, [1, 5, 9, V - 1]] = [-np.inf, np.float32(3e38), np.float32(-3e38), np.float32(1e30)]
    return lg


def _check(handle, lg, csr, automaton, hists, V, with_ts, form, **kw):
    eot, tsb = GEOMETRY[V]
    skipped = [r for r in range(len(hists)) if kw.get("done") and kw["done"][r // kw.get("K", 1)]]
    want = ar.automaton_rows(lg, csr, hists, eot, tsb, with_ts, skipped)
    for staging in (0, 1, 2):
        got = ar.rows_gpu(handle, lg, hists, automaton, eot, tsb, with_ts, form, staging=staging, **kw)
        assert np.array_equal(ar.bits(got), ar.bits(want)), (staging, np.argwhere(ar.bits(got) != ar.bits(want))[:8])
    return want


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("with_ts", [0, 1])
@pytest.mark.parametrize("name,V", [(n, V) for n, (_, Vs) in CASES.items() for V in Vs])
def test_rows_against_the_plain_walk(handle, name, V, with_ts, form):
    csr, launches = CASES[name][0](*GEOMETRY[V])
    automaton = ar.Automaton(V, csr)
    for i, hists in enumerate(launches):
        want = _check(handle, _logits(len(hists), V, i), csr, automaton, hists, V, with_ts, form)
        assert np.any(want[:, :GEOMETRY[V][1]] != -np.inf)            # (the launch keeps some text id somewhere)


@pytest.mark.parametrize("V", [67, 51866])
def test_skipped_rows_keep_every_bit(handle, V):
    """step form: the rows of a done chunk (K = 2); score form: rows without a target — untouched, also by the peeled head
    and tail stores of the rows beside them"""
    csr, launches = _loop2(*GEOMETRY[V])
    automaton, hists = ar.Automaton(V, csr), launches[2][:4]
    lg = _logits(4, V, 7)
    for done in ([0, 1], [1, 0]):
        _check(handle, lg, csr, automaton, hists, V, 0, 0, K=2, done=done)
    _check(handle, lg, csr, automaton, hists, V, 1, 1, done=[0, 1, 1, 0])
