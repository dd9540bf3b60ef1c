"""Small builders of regular languages over token ids, for automaton-constrained decoding (fwamd.h: fw_automaton_create;
backend.Whisper.automaton, generate(automaton=...), transcribe(allowed_grammar=...)).

    digits = Grammar.phrases([[15], [16], [17]])                    # one of these phrases (sequences of token ids)
    number = Grammar.repeat(digits, 4, 8)                            # four to eight of them
    timer  = Grammar.sequence([[[50, 51]], number, [[60], [61]]])    # slot after slot: a phrase list or a Grammar each
    either = number | timer

A phrase may also be a str: such a grammar is TEXT and must be bound to a tokenizer before use — `bind(encode)` gives
the same grammar over ids, every phrase encoded as encode(" " + phrase.strip()), the convention of boost_phrases and
allowed_phrases; transcribe(allowed_grammar=) binds for its caller.

A grammar compiles (NFA -> subset construction -> trim -> minimise) to ONE deterministic automaton, the smallest of its
language (so that a phrase list shares its suffixes and fits the engine's state limit), whose states are numbered in
breadth-first order from the start state, out-edges by ascending token: equal arguments give equal arrays, and with them
byte-equal engine tables, which is what lets two calls share a decode run."""
from collections import deque
from typing import Callable, Dict, List, Sequence, Tuple


class Grammar:
    def __init__(self, kind: str, parts: tuple):
        self._kind, self._parts = kind, parts
        self._dfa = None

    # ---- builders -----------------------------------------------------------------------
    @staticmethod
    def phrases(phrases: Sequence) -> "Grammar":
        """exactly one of `phrases`: each a sequence of token ids, or a str (see bind)"""
        if isinstance(phrases, (str, bytes)):
            raise ValueError("phrases must be a sequence of phrases, not one string")
        return Grammar("phrases", tuple(p if isinstance(p, str) else tuple(int(t) for t in p) for p in phrases))

    @staticmethod
    def sequence(slots: Sequence) -> "Grammar":
        """one string of every slot, in order; a slot is a Grammar or a phrase list"""
        return Grammar("sequence", tuple(s if isinstance(s, Grammar) else Grammar.phrases(s) for s in slots))

    @staticmethod
    def repeat(g: "Grammar", min_count: int, max_count: int) -> "Grammar":
        """min_count .. max_count strings of g, back to back"""
        if not isinstance(g, Grammar):
            g = Grammar.phrases(g)
        if not 0 <= min_count <= max_count or max_count < 1:
            raise ValueError(f"repeat counts {min_count} .. {max_count}: need 0 <= min_count <= max_count, max_count >= 1")
        return Grammar("repeat", (g, int(min_count), int(max_count)))

    def __or__(self, other: "Grammar") -> "Grammar":
        if not isinstance(other, Grammar):
            return NotImplemented
        return Grammar("or", (self, other))

    def bind(self, encode: Callable[[str], Sequence[int]]) -> "Grammar":
        """the same grammar over ids: every str phrase p becomes encode(" " + p.strip())"""
        if self._kind == "phrases":
            return Grammar.phrases([encode(" " + p.strip()) if isinstance(p, str) else p for p in self._parts])
        return Grammar(self._kind, tuple(p.bind(encode) if isinstance(p, Grammar) else p for p in self._parts))

    # ---- NFA fragments: states are ints, edges (state, token | None, state) with None = epsilon ----
    def _fragment(self, edges: list, new_state) -> Tuple[int, int]:
        """adds this grammar to `edges`; returns its (entry, exit) states"""
        a, b = new_state(), new_state()
        if self._kind == "phrases":
            for p in self._parts:
                if isinstance(p, str):
                    raise ValueError(f"the grammar holds the text phrase {p!r}: bind() it to a tokenizer first")
                s = a
                for t in p:
                    nxt = new_state()
                    edges.append((s, t, nxt))
                    s = nxt
                edges.append((s, None, b))
        elif self._kind == "or":
            for g in self._parts:
                x, y = g._fragment(edges, new_state)
                edges.append((a, None, x))
                edges.append((y, None, b))
        else:
            if self._kind == "sequence":
                items = [(g, True) for g in self._parts]
            else:   # repeat: max_count copies, the last max_count - min_count of which may be skipped
                g, lo, hi = self._parts
                items = [(g, i < lo) for i in range(hi)]
            s = a
            for g, required in items:
                x, y = g._fragment(edges, new_state)
                edges.append((s, None, x))
                if not required:
                    edges.append((s, None, b))
                s = y
            edges.append((s, None, b))
        return a, b

    def _compile(self) -> Tuple[List[Dict[int, int]], List[bool]]:
        """the trim DFA: (out-edges per state as {token: target}, accepting per state), state 0 the start state"""
        if self._dfa is not None:
            return self._dfa
        edges, count = [], [0]

        def new_state():
            count[0] += 1
            return count[0] - 1
        start, final = self._fragment(edges, new_state)
        eps = [[] for _ in range(count[0])]
        step = [[] for _ in range(count[0])]
        for s, t, to in edges:
            (eps[s] if t is None else step[s]).append(to if t is None else (t, to))

        def closure(states):
            seen, stack = set(states), list(states)
            while stack:
                for to in eps[stack.pop()]:
                    if to not in seen:
                        seen.add(to)
                        stack.append(to)
            return frozenset(seen)
        # subset construction
        first = closure([start])
        index, subsets, trans = {first: 0}, [first], []
        i = 0
        while i < len(subsets):
            by_token: Dict[int, set] = {}
            for s in subsets[i]:
                for t, to in step[s]:
                    by_token.setdefault(t, set()).add(to)
            row = {}
            for t, tos in by_token.items():
                nxt = closure(tos)
                if nxt not in index:
                    index[nxt] = len(subsets)
                    subsets.append(nxt)
                row[t] = index[nxt]
            trans.append(row)
            i += 1
        accepting = [final in sub for sub in subsets]
        # trim: keep the states from which an accepting one can be reached (all are reachable by construction)
        back = [[] for _ in subsets]
        for s, row in enumerate(trans):
            for to in row.values():
                back[to].append(s)
        live, stack = set(), [s for s, acc in enumerate(accepting) if acc]
        live.update(stack)
        while stack:
            for s in back[stack.pop()]:
                if s not in live:
                    live.add(s)
                    stack.append(s)
        if 0 not in live:
            raise ValueError("the grammar accepts no string at all")
        trans = [{t: to for t, to in row.items() if to in live} for row in trans]
        # minimise (partition refinement: states of one class accept alike and go to the same classes on the same ids), so
        # that the automaton is the language's smallest — a phrase list shares its suffixes, 128 phrases of 32 ids fit
        # the engine's state limit (other spellings of a language then compile alike too: a side effect, not a promise)
        cls = [int(a) for a in accepting]
        while True:
            sig = {}
            new = [sig.setdefault((cls[s], tuple(sorted((t, cls[to]) for t, to in trans[s].items()))), len(sig))
                   for s in range(len(trans))]
            if len(sig) == len(set(cls)):
                break
            cls = new
        rep = {}
        for s in sorted(live):
            rep.setdefault(cls[s], s)
        trans = [{t: rep[cls[to]] for t, to in row.items()} for row in trans]
        live = set(rep.values())
        # number breadth-first from the start state, out-edges by ascending token
        start = rep[cls[0]]
        order, number, queue = [start], {start: 0}, deque([start])
        while queue:
            s = queue.popleft()
            for t in sorted(trans[s]):
                to = trans[s][t]
                if to in live and to not in number:
                    number[to] = len(order)
                    order.append(to)
                    queue.append(to)
        self._dfa = ([{t: number[to] for t, to in sorted(trans[s].items()) if to in live} for s in order],
                     [accepting[s] for s in order])
        return self._dfa

    # ---- the language -------------------------------------------------------------------
    def _state_after(self, ids):
        out, _ = self._compile()
        s = 0
        for t in ids:
            s = out[s].get(int(t))
            if s is None:
                return None
        return s

    def accepts(self, ids: Sequence[int]) -> bool:
        s = self._state_after(ids)
        return s is not None and self._compile()[1][s]

    def is_prefix(self, ids: Sequence[int]) -> bool:
        """whether some accepted string starts with ids (the automaton is trim: every state leads to an accepting one)"""
        return self._state_after(ids) is not None

    def csr(self):
        """the arrays of fw_automaton_create: (edge_offsets [states + 1], edge_tokens, edge_targets, accepting [states])"""
        out, acc = self._compile()
        offsets, tokens, targets = [0], [], []
        for row in out:
            tokens += list(row)
            targets += list(row.values())
            offsets.append(len(tokens))
        return offsets, tokens, targets, [int(a) for a in acc]
