"""Back-off n-gram language models over token ids, for shallow fusion (fwamd.h: fw_ngram_create; backend.Whisper.ngram_lm,
generate(lm=...), transcribe(language_model=...)).

An NgramLM holds the explicit n-grams of orders 1 .. N with natural-log probabilities and back-off weights, independent of
any vocabulary size: its symbols are token ids plus BOS ("<s>") and EOS ("</s>"), which Whisper.ngram_lm maps to the
engine's BOS symbol and to the model's <eot>.  from_arpa reads a model an LM toolkit wrote; train estimates a small one
here, for machines without a toolkit."""
import math
import os
from collections import Counter, defaultdict
from typing import Dict, Iterable, List, Sequence, Tuple

import numpy as np

BOS, EOS, UNK = "<s>", "</s>", "<unk>"
_LN10 = math.log(10.0)


class NgramLM:
    """grams[k - 1]: {n-gram of order k (a tuple of ids, BOS only first, EOS only last): (log p, log back-off)}, natural
    logs; unk_logprob: the value of an id without a unigram.  The unigram (BOS,) carries the back-off of the context [BOS]
    and log p = 0: BOS is never predicted."""

    def __init__(self, grams: List[Dict[tuple, Tuple[float, float]]], unk_logprob: float):
        if not 1 <= len(grams) <= 5:
            raise ValueError(f"an n-gram model of order {len(grams)}: orders 1 .. 5")
        self.grams, self.unk_logprob = grams, float(unk_logprob)

    @property
    def order(self) -> int:
        return len(self.grams)

    def score(self, context: Sequence, v) -> float:
        """log P(v | context) by the back-off recursion of fwamd.h, in double precision; context: ids, BOS first if at all"""
        context, acc = tuple(context), 0.0
        for k in range(min(self.order - 1, len(context)), 0, -1):
            hit = self.grams[k].get(context[-k:] + (v,))
            if hit is not None:
                return acc + hit[0]
            acc += self.grams[k - 1].get(context[-k:], (0.0, 0.0))[1]
        return acc + self.grams[0].get((v,), (self.unk_logprob, 0.0))[0]

    def arrays(self, n_vocab: int, eos_id: int):
        """the arguments of fw_ngram_create: (counts [order], ids, logprobs, backoffs); BOS -> n_vocab, EOS -> eos_id"""
        sym = {BOS: int(n_vocab), EOS: int(eos_id)}
        counts, ids, lp, bo = [], [], [], []
        for level in self.grams:
            counts.append(len(level))
            for gram, (p, b) in level.items():
                ids.extend(sym.get(w, w) for w in gram)
                lp.append(p)
                bo.append(b)
        return (np.asarray(counts, dtype=np.int32), np.asarray(ids, dtype=np.int32), np.asarray(lp, dtype=np.float32),
                np.asarray(bo, dtype=np.float32))

    @classmethod
    def from_arpa(cls, path_or_text: str) -> "NgramLM":
        """An ARPA file (or its text) whose words are decimal token ids plus <s>, </s> and <unk>; log10 becomes natural log.
        <unk>'s unigram gives unk_logprob (-99 log10 without one); n-grams of higher order that hold <unk> are dropped, and
        the unigram <s> keeps its back-off only."""
        text = path_or_text
        if "\n" not in text and os.path.exists(text):
            with open(text) as f:
                text = f.read()
        grams, unk, k = [], -99.0 * _LN10, 0
        for line in text.splitlines():
            line = line.strip()
            if not line or line == "\\data\\" or line.startswith("ngram "):
                continue
            if line == "\\end\\":
                break
            if line.startswith("\\") and line.endswith("-grams:"):
                k = int(line[1:-7])
                if k != len(grams) + 1:
                    raise ValueError(f"ARPA section {line} out of order")
                grams.append({})
                continue
            f = line.split()
            if k == 0 or len(f) not in (k + 1, k + 2):
                raise ValueError(f"ARPA line not understood: {line!r}")
            words, p = f[1:k + 1], float(f[0]) * _LN10
            b = float(f[k + 1]) * _LN10 if len(f) == k + 2 else 0.0
            if UNK in words:
                if k == 1:
                    unk = p
                continue
            gram = tuple(w if w in (BOS, EOS) else int(w) for w in words)
            grams[k - 1][gram] = (0.0 if gram == (BOS,) else p, b)
        return cls(grams, unk)

    @classmethod
    def train(cls, token_id_sequences: Iterable[Sequence[int]], order: int, discount: float = 0.75) -> "NgramLM":
        """A plain absolute-discounting back-off estimate from sequences of token ids (each becomes <s> ids </s>): every
        seen n-gram gives up `discount` of its count, a context's back-off weight hands the mass so freed to the lower
        order, normalised over what the context did not see; at the unigram level it goes to <unk>, so that every
        context's distribution over the seen ids, </s> and <unk> sums to 1.  NOT a replacement for KenLM or SRILM — no
        modified Kneser-Ney, no pruning, no interpolation: it makes the fusion usable where no toolkit is."""
        if not 1 <= order <= 5 or not 0.0 < discount < 1.0:
            raise ValueError("order in [1, 5] and discount in (0, 1)")
        counts = [Counter() for _ in range(order)]
        for seq in token_id_sequences:
            s = (BOS,) + tuple(int(t) for t in seq) + (EOS,)
            for k in range(1, order + 1):
                counts[k - 1].update(s[i:i + k] for i in range(0 if k > 1 else 1, len(s) - k + 1))
        total = sum(counts[0].values())
        if total == 0:
            raise ValueError("no training text")
        lm = cls([{g: (math.log((c - discount) / total), 0.0) for g, c in counts[0].items()}],
                 math.log(discount * len(counts[0]) / total))
        for k in range(2, order + 1):
            followers = defaultdict(list)
            for g, c in counts[k - 1].items():
                followers[g[:-1]].append((g[-1], c))
            level = {}
            for ctx, fol in followers.items():
                n = sum(c for _, c in fol)
                for w, c in fol:
                    level[ctx + (w,)] = (math.log((c - discount) / n), 0.0)
                lower = sum(math.exp(lm.score(ctx[1:], w)) for w, _ in fol)
                p, _ = lm.grams[k - 2].get(ctx, (0.0, 0.0))     # ((<s>,) has no unigram of its own)
                lm.grams[k - 2][ctx] = (p, math.log(discount * len(fol) / n / (1.0 - lower)))
            lm.grams.append(level)
        return lm
