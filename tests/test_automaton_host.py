"""Host side of automaton-constrained decoding, no GPU: fw_automaton_create's validation and table, the plain C++ walk of
the compiled table, and grammar.py's builders against brute-force enumeration of their (finite) languages."""
import itertools

import numpy as np
import pytest

import automaton_refs as ar
from faster_whisper_amd.grammar import Grammar

GOOD = ([0, 2, 3, 3], [1, 4, 2], [1, 2, 2], [0, 0, 1])     # 0 -1-> 1, 0 -4-> 2, 1 -2-> 2, state 2 accepting


def _with(i, value):
    csr = [list(a) for a in GOOD]
    csr[i] = value
    return csr


@pytest.mark.parametrize("message,n_vocab,csr", [
    ("n_vocab 0", 0, GOOD),
    ("0 states", 9, ([0], [], [], [])),
    ("4097 states", 9, ([0] + [1] * 4097, [1], [0], [1] * 4097)),
    ("more than 8192 edges", 9000, ([0, 8193], list(range(8193)), [0] * 8193, [1])),
    (r"edge_offsets\[0\] = 1", 9, _with(0, [1, 2, 3, 3])),
    ("edge_offsets decrease at state 1", 9, _with(0, [0, 2, 1, 3])),
    ("state 0: id 1 follows id 4", 9, _with(1, [4, 1, 2])),
    ("state 0: id 1 follows id 1", 9, _with(1, [1, 1, 2])),
    ("state 0: edge id 4 outside", 4, GOOD),
    ("state 0, id 4: target 3 outside", 9, _with(2, [1, 3, 2])),
    ("state 2 cannot be reached", 9, ([0, 1, 1, 2], [1, 2], [1, 1], [0, 1, 0])),
    ("no accepting state can be reached from state 2", 9, _with(3, [0, 1, 0])),
])
def test_create_refuses(message, n_vocab, csr):
    with pytest.raises(ValueError, match=message):
        ar.Automaton(n_vocab, csr)


def test_create_refuses_null_pointers():
    from faster_whisper_amd import _lib
    assert _lib.load().fw_automaton_create(9, 1, None, None, None, None, None) == -1


def test_equal_arguments_give_equal_tables_and_the_host_walk_follows_them():
    a, b = ar.Automaton(9, GOOD), ar.Automaton(9, [list(x) for x in GOOD])
    assert np.array_equal(a.table(), b.table())
    assert not np.array_equal(a.table(), ar.Automaton(9, _with(3, [0, 1, 1])).table())
    lg = np.random.default_rng(0).standard_normal((6, 9)).astype(np.float32)
    hists = [[], [1], [8, 1, 7, 2], [4], [2], [1, 2, 2]]          # (ids 7 and 8 are timestamps below)
    for with_ts in (0, 1):
        got = ar.rows_host(lg, hists, a, 5, 7, with_ts)
        assert np.array_equal(ar.bits(got), ar.bits(ar.automaton_rows(lg, GOOD, hists, 5, 7, with_ts)))


A, B = Grammar.phrases([[0], [1, 2]]), Grammar.phrases([[2], [2, 0], []])


def _cat(x, y):
    return {p + q for p in x for q in y}


LA, LB = {(0,), (1, 2)}, {(2,), (2, 0), ()}
BUILDERS = {
    "phrases": (A, LA),
    "phrases with a prefix and the empty phrase": (B, LB),
    "sequence": (Grammar.sequence([A, [[1]], B]), _cat(_cat(LA, {(1,)}), LB)),
    "repeat 1..2": (Grammar.repeat(A, 1, 2), LA | _cat(LA, LA)),
    "repeat 0..3": (Grammar.repeat([[1]], 0, 3), {(), (1,), (1, 1), (1, 1, 1)}),
    "repeat 2..2 of a union": (Grammar.repeat(A | B, 2, 2), _cat(LA | LB, LA | LB)),
    "or": (A | Grammar.sequence([B, A]), LA | _cat(LB, LA)),
}


@pytest.mark.parametrize("name", list(BUILDERS))
def test_builders_against_enumeration(name):
    g, language = BUILDERS[name]
    for n in range(5):
        for s in itertools.product(range(3), repeat=n):
            assert g.accepts(s) == (s in language), s
            assert g.is_prefix(s) == any(w[:n] == s for w in language), s
    # the arrays are what fw_automaton_create takes (deterministic, trim), and building twice gives the same ones
    ar.Automaton(3, g.csr())
    assert g.csr() == Grammar(g._kind, g._parts).csr()


def test_text_phrases_are_bound_per_slot_element():
    g = Grammar.sequence([["call "], [" bob", "eve"]])
    with pytest.raises(ValueError):
        g.csr()
    bound = g.bind(lambda text: [ord(c) for c in text])
    assert bound.accepts([ord(c) for c in " call bob"]) and bound.accepts([ord(c) for c in " call eve"])
    with pytest.raises(ValueError):
        Grammar.phrases([]).csr()                              # the empty language


def test_allowed_grammar_is_bound_once_and_handed_to_every_generate_call():
    """transcribe_many(allowed_grammar=) on the scripted backend: ONE automaton for both recordings and every rung, built
    from the grammar bound to the tokenizer; together with allowed_phrases it is a ValueError before anything is decoded"""
    from faster_whisper_amd import get_config
    from oracle import micro_tokenizer
    from test_decode_extras_host import LADDER, ExtrasBackend, _audio
    from test_host_golden import make_model

    class Backend(ExtrasBackend):
        built, got = [], []

        def automaton(self, grammar):
            self.built.append(grammar)
            return grammar

        def generate(self, enc, prompts, *, automaton=None, **kw):
            self.got.append(automaton)
            return super().generate(enc, prompts, **kw)
    hf_tok = micro_tokenizer.build()
    m = make_model(get_config("micro"), hf_tok)
    m.model = Backend(get_config("micro"), hf_tok)
    g = Grammar.sequence([[" the quick"], ["brown fox ", "dog"]])
    assert len(m.transcribe_many([_audio(4), _audio(5, 4)], allowed_grammar=g, **LADDER)) == 2
    bound, = Backend.built
    assert len(Backend.got) >= 6 and all(a is bound for a in Backend.got)
    enc = m.make_tokenizer().encode
    assert bound.accepts(enc(" the quick") + enc(" brown fox")) and not bound.accepts(enc(" the quick"))
    with pytest.raises(ValueError, match="exclude each other"):
        m.transcribe(_audio(4), allowed_grammar=g, allowed_phrases=["dog"])
    assert len(Backend.built) == 1
