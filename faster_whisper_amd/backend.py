"""`ctranslate2.models.Whisper`-compatible front of the MI355X engine.

This is the host-side mirror of the reference's backend interface, exactly as it is used
at the call sites in faster_whisper/transcribe.py:
    constructor :689-698, .is_multilingual/.n_mels/.device/.device_index :379,484,1394,
    .encode :1400, .generate :222-236 / :1446-1459, .detect_language :215,1193,1823,
    .align :1709-1715, StorageView.from_array :1875,
    WhisperGenerationResult(.sequences_ids,.scores,.no_speech_prob) :241-248,
    WhisperAlignmentResult(.alignments,.text_token_probs) :1718-1719.
Same names, argument meaning and error behaviour (ValueError for bad arguments,
RuntimeError otherwise).  All arithmetic happens in libfwamd.so (HIP, gfx950); this file
only marshals.
"""
import ctypes as C
import itertools
import json
import os
import queue
import threading
from typing import Dict, List, Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib
from .config import WhisperConfig, get_config
from .weights import synthetic_weights, weight_shapes

MAX_ALTERNATIVES = _lib.FW_MAX_ALTERNATIVES   # generate(return_alternatives=N): N at most

_COMPUTE_TYPES = {
    "default": _lib.COMPUTE_FLOAT16, "auto": _lib.COMPUTE_FLOAT16, "float16": _lib.COMPUTE_FLOAT16,
    "int8_float16": _lib.COMPUTE_INT8_FLOAT16, "int8": _lib.COMPUTE_INT8_FLOAT16,
}


class StorageView:
    """N-d tensor handle: either a borrowed host numpy array (from_array) or a
    device-resident encoder output owned by the engine."""

    def __init__(self, array: Optional[np.ndarray] = None, handle=None, owner=None, shape=None, parts=None):
        self._array = array
        self._handle = handle
        self._owner = owner  # the _Replica that produced the handle
        # an encoder output of more chunks than the engine's max_batch is a list of device tensors (CTranslate2
        # takes any batch size; the engine's workspaces are sized once)
        self._parts = parts
        if parts:
            shape = (sum(p._shape[0] for p in parts),) + tuple(parts[0]._shape[1:])
        self._shape = tuple(shape) if shape is not None else (tuple(array.shape) if array is not None else ())

    @classmethod
    def from_array(cls, array) -> "StorageView":
        array = np.asarray(array)
        if not array.flags["C_CONTIGUOUS"]:
            raise ValueError("StorageView.from_array requires a C-contiguous array")
        return cls(array=array)

    @property
    def shape(self):
        return list(self._shape)

    @property
    def device(self) -> str:
        return "cpu" if self._handle is None and not self._parts else "cuda"

    @property
    def dtype(self):
        return np.float32 if self._handle is None else np.float16

    def to_numpy(self) -> np.ndarray:
        """float32 copy on the host (for device tensors: the to_cpu path)."""
        if self._parts:
            return np.concatenate([p.to_numpy() for p in self._parts], axis=0)
        if self._handle is None:
            return np.asarray(self._array)
        out = np.empty(self._shape, dtype=np.float32)
        _lib.check(_lib.load().fw_tensor_to_host(self._owner.handle, self._handle, _lib.ptr(out)))
        return out

    def __array__(self, dtype=None, copy=None):
        a = self.to_numpy()
        return a.astype(dtype) if dtype is not None else a

    def __del__(self):
        if getattr(self, "_handle", None) is not None:
            try:
                _lib.load().fw_tensor_free(self._handle)
            except Exception:
                pass
            self._handle = None


class WhisperGenerationResult:
    def __init__(self, sequences_ids, scores, no_speech_prob, token_logprobs=None, end_logprobs=None):
        self.sequences_ids = sequences_ids
        self.sequences = [[str(t) for t in s] for s in sequences_ids]
        self.scores = scores
        self.no_speech_prob = no_speech_prob
        # generate(return_token_logprobs=True): token_logprobs[h][i] = log-prob of sequences_ids[h][i] under the
        # processed distribution (after the logits rules), end_logprobs[h] = that of the closing <eot> (0.0: cut at
        # the budget).  Empty lists when not requested.
        self.token_logprobs = token_logprobs if token_logprobs is not None else []
        self.end_logprobs = end_logprobs if end_logprobs is not None else []
        # generate(return_alternatives=N): token_alternatives[h][i] = the N most likely (id, log-prob) pairs of the
        # distribution sequences_ids[h][i] was chosen from (log-prob descending, id ascending; (0, -inf) where fewer than N
        # ids were left), end_alternatives[h] = those of the step that produced the closing <eot>, None when the
        # hypothesis was cut at the budget.  Empty lists when not requested.
        self.token_alternatives = []
        self.end_alternatives = []

    def __repr__(self):
        return (f"WhisperGenerationResult(sequences_ids={self.sequences_ids}, scores={self.scores}, "
                f"no_speech_prob={self.no_speech_prob})")


class WhisperAlignmentResult:
    def __init__(self, alignments, text_token_probs):
        self.alignments = alignments
        self.text_token_probs = text_token_probs


class WhisperScoringResult:
    """Whisper.score for one chunk.  Per candidate sequence h: token_logprobs[h][i] = log-prob of the given token i,
    end_logprobs[h] = that of the <eot> that would close the sequence, best_ids[h] / best_logprobs[h] = the arg-max of
    the same distribution at every position, the <eot> position last (len(sequence) + 1 entries)."""

    def __init__(self, sequences_ids, token_logprobs, end_logprobs, best_ids, best_logprobs):
        self.sequences_ids = sequences_ids
        self.token_logprobs = token_logprobs
        self.end_logprobs = end_logprobs
        self.best_ids = best_ids
        self.best_logprobs = best_logprobs

    def cum_logprob(self, h: int = 0) -> float:
        """the tokens' values, then the <eot>'s, added in order in float32: generate's cumulative log-prob"""
        acc = np.float32(0.0)
        for v in self.token_logprobs[h] + [self.end_logprobs[h]]:
            acc = np.float32(acc + np.float32(v))
        return float(acc)

    def score(self, h: int = 0, length_penalty: float = 1) -> float:
        """generate's normalised score of candidate h: cum_logprob / len ** length_penalty (float32, as the engine)"""
        n = max(1, len(self.sequences_ids[h]))
        denom = np.float32(n) ** np.float32(length_penalty) if length_penalty != 0 else np.float32(1.0)
        return float(np.float32(self.cum_logprob(h)) / np.float32(denom))

    def __repr__(self):
        return (f"WhisperScoringResult(sequences_ids={self.sequences_ids}, token_logprobs={self.token_logprobs}, "
                f"end_logprobs={self.end_logprobs})")


class _PhraseList:
    """What BoostList and ConstraintList share: the ragged packing of the phrases, the engine's handle and its release, the
    type check of the keyword that takes the list.  A subclass names its keyword, what the feature is called in messages,
    and its create / free symbols."""
    _keyword = _feature = _create = _free = None

    def _compile(self, n_vocab: int, phrases, *per_phrase):
        lib = _lib.load()
        if not hasattr(lib, self._create):   # an older build loaded through FWAMD_LIB
            raise RuntimeError(f"this libfwamd.so has no {self._create}: {self._feature} needs a current build")
        flat, offs = _ragged([np.asarray(p, dtype=np.int32) for p in phrases], np.int32, np.int32)
        self.n_vocab = int(n_vocab)
        self.n_phrases = len(phrases)
        self._handle = C.c_void_p()
        _lib.check(getattr(lib, self._create)(self.n_vocab, _lib.as_i32p(flat), _lib.as_i32p(offs), len(phrases),
                                              *per_phrase, C.byref(self._handle)))

    def __len__(self):
        return self.n_phrases

    def __del__(self):
        if getattr(self, "_handle", None):
            try:
                getattr(_lib.load(), self._free)(self._handle)
            except Exception:
                pass
            self._handle = None

    @classmethod
    def _handle_of(cls, value):
        """the handle of a keyword's value: None, or a list of this class (TypeError)"""
        if value is None:
            return None
        if not isinstance(value, cls):
            raise TypeError(f"{cls._keyword} must be a {cls.__name__} (Whisper.{cls._keyword}_list) or None")
        return value._handle


class BoostList(_PhraseList):
    """A validated, compiled list of phrases to boost (fwamd.h: fw_boost_create): phrases[j] is a sequence of token ids,
    boosts[j] the float added to the logit of the phrase's next token wherever the generated history ends with the tokens
    in front of it (the first token: at every step).  Where several phrases ask for one id the largest boost counts, not the
    sum; the decoding rules run after the boost and still win.  Host-only: needs no device.  Whisper.boost_list builds one
    for the model's vocabulary; pass it as generate(boost=...) / score(boost=...)."""
    _keyword, _feature, _create, _free = "boost", "phrase boosting", "fw_boost_create", "fw_boost_free"

    def __init__(self, n_vocab: int, phrases: Sequence[Sequence[int]], boosts: Sequence[float]):
        phrases = [list(p) for p in phrases]
        boosts = list(boosts)
        if len(phrases) != len(boosts):
            raise ValueError(f"got {len(phrases)} phrases and {len(boosts)} boosts")
        b = np.asarray(boosts, dtype=np.float32).reshape(-1)
        self._compile(n_vocab, phrases, _lib.as_f32p(b) if b.size else None)


class ConstraintList(_PhraseList):
    """A validated, compiled list of the phrases a decode may produce (fwamd.h: fw_constraint_create): phrases[j] is a
    sequence of token ids.  At every step the ids that continue no listed phrase after the row's generated text are set to
    -inf in front of the decoding rules, and <eot> is allowed only where a phrase is complete: a hypothesis with a finite
    score that closes on <eot> is, its timestamps apart, one phrase of the list.  Duplicates and phrases that are prefixes
    of others are valid; the list is a set (order and repeats do not matter).  Host-only: needs no device.
    Whisper.constraint_list builds one for the model's vocabulary; pass it as generate(constraint=...) /
    score(constraint=...).  An empty list constrains nothing."""
    _keyword, _feature, _create, _free = "constraint", "constrained decoding", "fw_constraint_create", "fw_constraint_free"

    def __init__(self, n_vocab: int, phrases: Sequence[Sequence[int]]):
        self._compile(n_vocab, [list(p) for p in phrases])


def _require_symbols(lib, needs) -> None:
    """needs: (used, symbol, what it serves) in the order the features were added.  A build loaded through FWAMD_LIB that
    lacks the symbol of a feature the call uses cannot serve the call (RuntimeError)."""
    for used, symbol, what in needs:
        if used and not hasattr(lib, symbol):
            raise RuntimeError(f"this libfwamd.so has no {symbol}: {what} a current build")


def _generate_call(lib, head, outs, lp, alt, n_alt, top_k, top_p, boost_h, constraint_h):
    """The engine entry point of a generate call and its argument list: the OLDEST symbol that can express the call, so a
    build that lacks newer ones still serves every call it can.  head: (model, encoder output, prompts, offsets, B, options);
    outs: (ids, lens, scores, no-speech probabilities); lp: the two log-prob arrays, alt: the four alternative arrays
    (None where the call does not ask for them).  Every entry's argument order is stated here and nowhere else."""
    trunc = top_k != 0 or top_p != 1.0   # (NaN included: the engine refuses it)
    want_lp = lp[0] is not None
    _require_symbols(lib, ((boost_h is not None, "fw_generate_boost", "phrase boosting needs"),
                           (constraint_h is not None, "fw_generate_constrain", "constrained decoding needs"),
                           (trunc, "fw_generate_trunc", "top_k / top_p need"),
                           (n_alt, "fw_generate_alt", "per-token log-probabilities and alternatives need"),
                           (want_lp, "fw_generate_lp", "per-token log-probabilities need")))
    if constraint_h is not None:
        return lib.fw_generate_constrain, (*head, top_k, top_p, n_alt, boost_h, constraint_h, *outs, *lp, *alt)
    if trunc:
        return lib.fw_generate_trunc, (*head, top_k, top_p, n_alt, boost_h, *outs, *lp, *alt)
    if boost_h is not None:
        return lib.fw_generate_boost, (*head, n_alt, boost_h, *outs, *lp, *alt)
    if n_alt:
        return lib.fw_generate_alt, (*head, n_alt, *outs, *lp, *alt)
    if want_lp:
        return lib.fw_generate_lp, (*head, *outs, *lp)
    return lib.fw_generate, (*head, *outs)


def _score_call(lib, head, outs, boost_h, constraint_h):
    """as _generate_call, for score().  head: (model, encoder output, prompts, offsets, targets, offsets, B, H, rules)"""
    _require_symbols(lib, ((True, "fw_score", "scoring needs"),
                           (boost_h is not None, "fw_score_boost", "phrase boosting needs"),
                           (constraint_h is not None, "fw_score_constrain", "constrained decoding needs")))
    if constraint_h is not None:
        return lib.fw_score_constrain, (*head, boost_h, constraint_h, *outs)
    if boost_h is not None:
        return lib.fw_score_boost, (*head, boost_h, *outs)
    return lib.fw_score, (*head, *outs)


class _Replica:
    """one fw_model on one GPU"""

    def __init__(self, cfg: WhisperConfig, weights: Optional[Dict[str, np.ndarray]], compute_type: int,
                 device_index: int, max_batch: int, max_beam: int, blob_dev: Optional[Tuple[int, int]] = None):
        lib = _lib.load()
        self.cfg = cfg
        self.device_index = device_index
        self.handle = C.c_void_p()
        ccfg = cfg.to_c()
        if blob_dev is not None:
            ptr, nbytes = blob_dev
            _lib.check(lib.fw_model_create_from_blob_dev(C.byref(ccfg), C.c_void_p(ptr), nbytes, compute_type,
                                                         device_index, max_batch, max_beam, C.byref(self.handle)))
            return
        arr, keep = make_weight_array(cfg, weights)
        _lib.check(lib.fw_model_create(C.byref(ccfg), arr, len(keep), compute_type, device_index, max_batch,
                                       max_beam, C.byref(self.handle)))

    def close(self):
        if self.handle:
            _lib.load().fw_model_free(self.handle)
            self.handle = C.c_void_p()


def make_weight_array(cfg: WhisperConfig, weights: Dict[str, np.ndarray]):
    shapes = weight_shapes(cfg)
    missing = [n for n in shapes if n not in weights]
    if missing:
        raise ValueError(f"missing weights: {missing[:5]}{'...' if len(missing) > 5 else ''}")
    arr = (_lib.FwWeight * len(shapes))()
    keep = []
    for i, (name, shape) in enumerate(shapes.items()):
        a = weights[name]
        if a.dtype not in (np.float16, np.float32):
            a = a.astype(np.float32)
        a = np.ascontiguousarray(a)
        if tuple(a.shape) != tuple(shape):
            raise ValueError(f"weight {name}: shape {a.shape}, expected {shape}")
        keep.append(a)
        arr[i].name = name.encode()
        arr[i].data = a.ctypes.data
        arr[i].dtype = _lib.FW_DT_F16 if a.dtype == np.float16 else _lib.FW_DT_F32
        arr[i].ndim = a.ndim
        for k in range(a.ndim):
            arr[i].dims[k] = a.shape[k]
    return arr, keep


def pack_blob(cfg: WhisperConfig, weights: Dict[str, np.ndarray], compute_type: int = 0) -> np.ndarray:
    """Host image of the device weight blob (what rank 0 broadcasts over RCCL at load)."""
    lib = _lib.load()
    arr, keep = make_weight_array(cfg, weights)
    size = C.c_int64()
    h = C.c_void_p()
    ccfg = cfg.to_c()
    _lib.check(lib.fw_pack_blob_size(C.byref(ccfg), arr, len(keep), compute_type, C.byref(size), C.byref(h)))
    out = np.empty(size.value, dtype=np.uint8)
    try:
        _lib.check(lib.fw_pack_blob_copy(h, _lib.ptr(out), size.value))
    finally:
        lib.fw_pack_blob_free(h)
    return out


def load_model_dir(path: str) -> Tuple[WhisperConfig, Dict[str, np.ndarray]]:
    """fwamd model directory: fwamd_config.json + weights.safetensors (see save_model_dir)."""
    cfg_path = os.path.join(path, "fwamd_config.json")
    if not os.path.isfile(cfg_path):
        if os.path.isfile(os.path.join(path, "model.bin")):
            # a CTranslate2 converted directory (what the reference downloads, utils.py:91-97)
            from .ct2_format import load_ct2_model_dir
            return load_ct2_model_dir(path)
        raise RuntimeError(f"{path}: neither fwamd_config.json nor model.bin found")
    with open(cfg_path) as f:
        j = json.load(f)
    j["suppress_begin"] = tuple(j.get("suppress_begin", ()))
    j["alignment_heads"] = [tuple(x) for x in j.get("alignment_heads", [])]
    cfg = WhisperConfig(**j)
    from safetensors.numpy import load_file
    weights = load_file(os.path.join(path, "weights.safetensors"))
    return cfg, weights


def save_model_dir(path: str, cfg: WhisperConfig, weights: Dict[str, np.ndarray]):
    from dataclasses import asdict
    from safetensors.numpy import save_file
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "fwamd_config.json"), "w") as f:
        json.dump(asdict(cfg), f)
    save_file({k: np.ascontiguousarray(v) for k, v in weights.items()}, os.path.join(path, "weights.safetensors"))


def call_seed(n: int) -> int:
    """seed of the n-th sampling call of a model (splitmix64 of the call counter)"""
    z = (n * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return z ^ (z >> 31)


def _splitmix64(z: int) -> int:
    z = (z + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return z ^ (z >> 31)


def attempt_seed(base: int, seek: int, temperature_index: int) -> int:
    """seed of ONE sampled fallback attempt of a transcribe(sampling_seed=base) call: the attempt at rung
    `temperature_index` of the temperature ladder for the window that starts at frame `seek`.  Three chained splitmix64
    steps (base, then seek, then the rung, each added to the state before the next mix): a pure function of its
    arguments, so the attempt draws the same samples whatever ran before it or runs beside it, and two windows or two
    rungs of one recording never share a seed by construction of the mix (64-bit collisions aside)."""
    z = _splitmix64(int(base) & 0xFFFFFFFFFFFFFFFF)
    z = _splitmix64(z ^ (int(seek) & 0xFFFFFFFFFFFFFFFF))
    return _splitmix64(z ^ (int(temperature_index) & 0xFFFFFFFFFFFFFFFF))


def recording_seed(base: int, i: int) -> int:
    """sampling_seed of recording `i` of a transcribe_many(sampling_seed=base) call: splitmix64 of the mixed base with
    the recording's index folded in (under a constant that keeps it apart from attempt_seed's chain).  result[i] of that
    call is transcribe(audios[i], sampling_seed=recording_seed(base, i))."""
    z = _splitmix64((int(base) & 0xFFFFFFFFFFFFFFFF) ^ 0xD1B54A32D192ED03)
    return _splitmix64(z ^ (int(i) & 0xFFFFFFFFFFFFFFFF))


class Whisper:
    """Drop-in for ctranslate2.models.Whisper on MI355X.

    model_path:  a fwamd model directory, or "synthetic:<geometry>[:seed=<n>]" for seeded
                 random weights of a known geometry (benchmark / tests).
    files:       optional in-memory model: {"config": WhisperConfig, "weights": {name: ndarray}}
                 (the reference forwards its `files=` argument here, transcribe.py:696).
    """

    def __init__(self, model_path: str, device: str = "auto", device_index: Union[int, List[int]] = 0,
                 compute_type: str = "default", intra_threads: int = 0, inter_threads: int = 1,
                 files: Optional[dict] = None, max_batch_size: int = 16, max_beam_size: int = 5,
                 blob_dev: Optional[Tuple[int, int]] = None, **kwargs):
        if device not in ("auto", "cuda", "gpu", "hip"):
            raise ValueError(
                f"unsupported device '{device}': this backend runs on AMD GPUs only (device='cuda'/'auto'); "
                "there is no CPU path")
        if compute_type not in _COMPUTE_TYPES:
            raise ValueError(f"unsupported compute_type '{compute_type}' (supported: float16, int8_float16)")
        # the RESOLVED type, as ctranslate2's `compute_type` property reports it ("int8" on a device with fp16 -> int8_float16)
        self._compute_type_name = {"default": "float16", "auto": "float16",
                                   "int8": "int8_float16"}.get(compute_type, compute_type)
        ct = _COMPUTE_TYPES[compute_type]
        if files and "config" in files:
            cfg, weights = files["config"], files.get("weights")
        elif isinstance(model_path, str) and model_path.startswith("synthetic:"):
            parts = model_path.split(":")
            cfg = get_config(parts[1])
            seed = 1234
            for p in parts[2:]:
                if p.startswith("seed="):
                    seed = int(p[5:])
            weights = None if blob_dev is not None else synthetic_weights(cfg, seed)
        else:
            cfg, weights = load_model_dir(model_path)
        self._cfg = cfg
        self._max_batch = int(max_batch_size)
        self._max_beam = int(max_beam_size)
        idx = [device_index] if isinstance(device_index, int) else list(device_index)
        self._device_index = idx
        self._lib = _lib.load()
        # one replica per (device, worker): the `inter_threads` workers of a device share ONE copy of the
        # weights in HBM and own a stream + workspaces each (CTranslate2 replica pool semantics,
        # transcribe.py:645-657), so concurrent transcribe() threads overlap on the GPU
        # The workers of a device form a DECODE GROUP (include/fwamd.h): they share one decode workspace sized
        # for all of their batches, and generate() calls that arrive concurrently are merged into one decode run
        # whose rows share every weight byte streamed per step.  decode_group=False keeps a decoder per worker.
        self._replicas = []
        decode_group = bool(kwargs.pop("decode_group", True))
        # merge_wait_ms: how long the leader of a decode run waits for workers that are still encoding
        # (fwamd.h: fw_model_set_merge_wait; None = one encoder pass, 0 = never: lowest latency per call)
        merge_wait_ms = kwargs.pop("merge_wait_ms", None)
        merge_fill = kwargs.pop("merge_fill_percent", None)
        for i in idx:
            primary = _Replica(cfg, weights, ct, i, max_batch_size, max_beam_size, blob_dev)
            self._replicas.append(primary)
            if inter_threads > 1:
                p, n = C.c_void_p(), C.c_int64()
                _lib.check(self._lib.fw_model_blob(primary.handle, C.byref(p), C.byref(n)))
                if decode_group:
                    _lib.check(self._lib.fw_model_set_decode_batch(primary.handle, inter_threads * max_batch_size))
                for _ in range(inter_threads - 1):
                    r = _Replica(cfg, None, ct, i, max_batch_size, max_beam_size, (p.value, n.value))
                    if decode_group:
                        _lib.check(self._lib.fw_model_join_decoder(r.handle, primary.handle))
                    self._replicas.append(r)
            if merge_wait_ms is not None or merge_fill is not None:
                _lib.check(self._lib.fw_model_set_merge_wait(primary.handle, -1 if merge_wait_ms is None else int(merge_wait_ms),
                                                             90 if merge_fill is None else int(merge_fill)))
        self._seed_counter = itertools.count(1)
        self._rr = itertools.count()
        self._tls = threading.local()
        self.inter_threads = len(self._replicas)   # batches the host drivers may keep in flight

    # ---- properties read by the reference host code -------------------------------------
    @property
    def is_multilingual(self) -> bool:
        return bool(self._cfg.is_multilingual)

    @property
    def n_mels(self) -> int:
        return self._cfg.n_mels

    @property
    def device(self) -> str:
        return "cuda"

    @property
    def device_index(self) -> List[int]:
        return list(self._device_index)

    @property
    def compute_type(self) -> str:
        return self._compute_type_name

    @property
    def num_languages(self) -> int:
        return self._cfg.n_langs

    @property
    def config(self) -> WhisperConfig:
        return self._cfg

    def blob(self, replica: int = 0) -> Tuple[int, int]:
        """(device pointer, bytes) of the packed weight blob of a device's primary replica (fwamd.h: fw_model_blob) — what
        rank 0 hands to sharding.broadcast_blob_dev and what `blob_dev=` takes on the other ranks"""
        p, n = C.c_void_p(), C.c_int64()
        _lib.check(self._lib.fw_model_blob(self._replicas[self._primary_of(replica)].handle, C.byref(p), C.byref(n)))
        return int(p.value), int(n.value)

    def set_decode_lanes(self, lanes: int):
        """decode runs a device's group may have in flight (fwamd.h: fw_model_set_decode_lanes): 2, or 1 for per-kernel timing"""
        for i in sorted({self._primary_of(r) for r in range(len(self._replicas))}):
            _lib.check(self._lib.fw_model_set_decode_lanes(self._replicas[i].handle, int(lanes)))

    def synchronize(self):
        """block until everything queued on the encoder and decode streams of every worker has finished"""
        for r in self._replicas:
            _lib.check(self._lib.fw_synchronize(r.handle))

    def decode_stats(self) -> dict:
        """counters of the decode group of device 0: how many generate() calls shared how many decode runs"""
        runs, reqs, chunks, mx = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int32()
        _lib.check(self._lib.fw_model_decode_stats(self._replicas[0].handle, C.byref(runs), C.byref(reqs),
                                                   C.byref(chunks), C.byref(mx)))
        return {"runs": runs.value, "requests": reqs.value, "chunks": chunks.value, "max_run_chunks": mx.value,
                "decode_batch": int(self._lib.fw_model_decode_batch(self._replicas[0].handle)),
                "run_capacity": int(self._lib.fw_model_run_capacity(self._replicas[0].handle))}

    def graph_captures(self) -> int:
        """step graphs the decode group of device 0 has captured since the model was created (fwamd_test.h:
        fw_test_graph_captures); -1 with an older build loaded through FWAMD_LIB, which does not count them"""
        if not hasattr(self._lib, "fw_test_graph_captures"):
            return -1
        n = C.c_int64()
        _lib.check(self._lib.fw_test_graph_captures(self._replicas[0].handle, C.byref(n)))
        return int(n.value)

    def dec_big_min_rows(self) -> int:
        """rows from which a decode run's linears take the GEMM-shaped kernel (bench.py prices them accordingly)"""
        return int(self._lib.fw_dec_big_min_rows())

    def dec_big_min_rows_of(self, role: int) -> int:
        """the same for one linear (0 qkv, 1 d x d, 2 ffn1, 3 ffn2) of THIS model's compute type: every linear has its own
        measured crossover (include/fwamd_test.h)"""
        if not hasattr(self._lib, "fw_dec_big_min_rows_of"):      # an older build loaded through FWAMD_LIB (A/B of two builds)
            return self.dec_big_min_rows()
        return int(self._lib.fw_dec_big_min_rows_of(int(role), 1 if self._compute_type_name == "int8_float16" else 0))

    def _replica_for(self, features: Optional[StorageView]) -> _Replica:
        if features is not None and features._owner is not None:
            return features._owner
        # thread affinity: a host thread keeps the replica it was first given (round-robin), so W
        # threads on W replicas never contend and an encoder output stays with its worker
        r = getattr(self._tls, "replica", None)
        if r is None:
            r = self._replicas[next(self._rr) % len(self._replicas)]
            self._tls.replica = r
        return r

    def _as_encoded(self, features) -> StorageView:
        """generate/detect_language/align accept an encoder output or raw features (like CTranslate2)."""
        if not isinstance(features, StorageView):
            features = StorageView.from_array(features)
        if features._handle is not None or features._parts:
            return features
        a = np.asarray(features._array)
        if a.ndim == 3 and a.shape[1] == self._cfg.n_audio_ctx and a.shape[2] == self._cfg.d_model:
            # encoder output that went through the host (to_cpu=True, transcribe.py:1392-1394)
            rep = self._replica_for(None)
            a = np.ascontiguousarray(a, dtype=np.float32)
            h = C.c_void_p()
            _lib.check(self._lib.fw_tensor_from_host(rep.handle, _lib.ptr(a), a.shape[0], C.byref(h)))
            return StorageView(handle=h, owner=rep, shape=a.shape)
        return self.encode(features)

    @staticmethod
    def _over_parts(enc: StorageView, call, *per_chunk) -> list:
        """call(part, *per_chunk arguments of the part's chunks) for every device tensor of an encoder output, in order;
        the per-chunk results concatenated (an output of at most max_batch chunks is its own single part)"""
        out, b0 = [], 0
        for part in enc._parts or [enc]:
            b1 = b0 + part._shape[0]
            out.extend(call(part, *(arg[b0:b1] for arg in per_chunk)))
            b0 = b1
        return out

    # ---- encode -------------------------------------------------------------------------
    def encode(self, features: StorageView, to_cpu: bool = False) -> StorageView:
        if not isinstance(features, StorageView):
            features = StorageView.from_array(features)
        a = features._array
        if a is None:
            raise ValueError("encode expects host features")
        if a.ndim != 3 or a.shape[1] != self._cfg.n_mels or a.shape[2] != 3000:
            raise ValueError(
                f"Invalid input features shape: expected an input with shape (B, {self._cfg.n_mels}, 3000), "
                f"but got an input with shape {tuple(a.shape)} instead")
        a = np.ascontiguousarray(a, dtype=np.float32)
        if a.shape[0] > self._max_batch:
            out = StorageView(parts=[self.encode(StorageView.from_array(a[i:i + self._max_batch]))
                                     for i in range(0, a.shape[0], self._max_batch)])
            return StorageView.from_array(out.to_numpy()) if to_cpu else out
        rep = self._replica_for(None)
        h = C.c_void_p()
        _lib.check(self._lib.fw_encode(rep.handle, _lib.ptr(a), a.shape[0], C.byref(h)))
        out = StorageView(handle=h, owner=rep, shape=(a.shape[0], self._cfg.n_audio_ctx, self._cfg.d_model))
        if to_cpu:
            return StorageView.from_array(out.to_numpy())
        return out

    def encode_pcm(self, chunks: Sequence[np.ndarray]) -> StorageView:
        """Fused resident path (not in CTranslate2): ragged PCM -> log-mel -> encoder on the GPU."""
        if len(chunks) > self._max_batch:
            return StorageView(parts=[self.encode_pcm(chunks[i:i + self._max_batch])
                                      for i in range(0, len(chunks), self._max_batch)])
        rep = self._replica_for(None)
        pcm, offs = _ragged(chunks, np.float32)
        h = C.c_void_p()
        _lib.check(self._lib.fw_encode_pcm(rep.handle, _lib.ptr(pcm), _lib.as_i64p(offs), len(chunks), C.byref(h)))
        return StorageView(handle=h, owner=rep, shape=(len(chunks), self._cfg.n_audio_ctx, self._cfg.d_model))

    def stage_pcm(self, chunks: Sequence[np.ndarray], replica: int = 0):
        """Copy ragged PCM chunks into HBM once; returns an opaque staged batch for encode_pcm_staged
        (bench.py: inputs are resident in HBM when the timed region starts)."""
        rep = self._replicas[replica]
        pcm, offs = _ragged(chunks, np.float32)
        dev = C.c_void_p()
        _lib.check(self._lib.fw_dev_alloc(rep.handle, pcm.nbytes, C.byref(dev)))
        _lib.check(self._lib.fw_dev_upload(rep.handle, dev, _lib.ptr(pcm), pcm.nbytes))
        return {"dev": dev, "offsets": offs, "B": len(chunks), "rep": rep}

    def free_staged(self, staged):
        _lib.check(self._lib.fw_dev_free(staged["rep"].handle, staged["dev"]))

    def encode_pcm_staged(self, staged) -> StorageView:
        # the staged PCM lives in HBM of the device: any worker replica of that device may consume it
        rep = self._replica_for(None)
        if rep.device_index != staged["rep"].device_index:
            rep = staged["rep"]
        h = C.c_void_p()
        _lib.check(self._lib.fw_encode_pcm_dev(rep.handle, staged["dev"], _lib.as_i64p(staged["offsets"]),
                                               staged["B"], C.byref(h)))
        return StorageView(handle=h, owner=rep, shape=(staged["B"], self._cfg.n_audio_ctx, self._cfg.d_model))

    def log_mel(self, chunks: Sequence[np.ndarray]) -> np.ndarray:
        """FeatureExtractor(chunk)[..., :-1] + pad_or_trim for a batch of chunks, on the GPU."""
        rep = self._replica_for(None)
        out = np.empty((len(chunks), self._cfg.n_mels, 3000), dtype=np.float32)
        for b0 in range(0, len(chunks), self._max_batch):      # the engine's workspaces hold max_batch_size chunks
            part = chunks[b0:b0 + self._max_batch]
            pcm, offs = _ragged(part, np.float32)
            _lib.check(self._lib.fw_logmel(rep.handle, _lib.ptr(pcm), _lib.as_i64p(offs), len(part),
                                           _lib.ptr(out[b0:b0 + len(part)]), None))
        return out

    def log_mel_full(self, waveform: np.ndarray) -> np.ndarray:
        rep = self._replica_for(None)
        w = np.ascontiguousarray(waveform, dtype=np.float32)
        nf = w.shape[0] // 160 + 1
        out = np.empty((self._cfg.n_mels, nf), dtype=np.float32)
        _lib.check(self._lib.fw_logmel_full(rep.handle, _lib.ptr(w), w.shape[0], _lib.ptr(out), nf))
        return out

    # ---- phrase boosting ----------------------------------------------------------------
    def boost_list(self, phrases: Sequence[Sequence[int]], boosts: Sequence[float]) -> BoostList:
        """A BoostList for this model's vocabulary: phrases[j] a sequence of token ids, boosts[j] its strength in logit
        units.  ValueError (fwamd.h: FW_BOOST_MAX_PHRASES / _LEN / _TOKENS): more than 1024 phrases, a phrase of no token or
        more than 32, more than 4096 tokens in all, an id outside the vocabulary, a boost that is not finite."""
        return BoostList(self._cfg.n_vocab, phrases, boosts)

    # ---- constrained decoding -----------------------------------------------------------
    def constraint_list(self, phrases: Sequence[Sequence[int]]) -> ConstraintList:
        """A ConstraintList for this model's vocabulary: phrases[j] a sequence of token ids.  ValueError (fwamd.h:
        FW_CONSTRAIN_MAX_PHRASES / _LEN / _TOKENS): more than 1024 phrases, a phrase of no token or more than 32, more than
        4096 tokens in all, an id outside the vocabulary.  What a generate / score call refuses of a list (an id from <eot>
        on, a suppressed id, ...) is checked by that call, against its own rules."""
        return ConstraintList(self._cfg.n_vocab, phrases)

    # ---- generate -----------------------------------------------------------------------
    def generate(self, features: StorageView, prompts: List[List[int]], *, asynchronous: bool = False,
                 beam_size: int = 5, patience: float = 1, num_hypotheses: int = 1, length_penalty: float = 1,
                 repetition_penalty: float = 1, no_repeat_ngram_size: int = 0, max_length: int = 448,
                 return_scores: bool = False, return_logits_vocab: bool = False, return_no_speech_prob: bool = False,
                 max_initial_timestamp_index: int = 50, suppress_blank: bool = True,
                 suppress_tokens: Optional[Sequence[int]] = (-1,), sampling_topk: int = 1,
                 sampling_temperature: float = 1, min_new_tokens: int = 0,
                 seed: Optional[int] = None, return_token_logprobs: bool = False,
                 return_alternatives: int = 0, boost: Optional[BoostList] = None, top_k: int = 0,
                 top_p: float = 1.0, constraint: Optional[ConstraintList] = None) -> List[WhisperGenerationResult]:
        """boost (not in CTranslate2): a BoostList (boost_list()) whose phrases are made more likely at the logit, in front
        of the decoding rules; None or an empty list: the call without it.
        top_k / top_p (not in CTranslate2's generate(); fwamd.h: fw_generate_trunc): limits on the draw of a SAMPLING call
        (beam_size 1, sampling_topk 0) — the top_k most likely tokens, then the nucleus holding top_p of their tempered
        mass.  0 / 1.0: no limit, and the call is the one it always was.  ValueError: top_k < 0, top_p outside (0, 1], a
        limit on a call that does not sample.  Token log-probs and alternatives stay those of the whole distribution.
        constraint (not in CTranslate2; fwamd.h: fw_generate_constrain): a ConstraintList (constraint_list()); every
        hypothesis is then, its timestamps apart, one phrase of the list (or a prefix of one when the budget cut it).  Runs
        behind the boost and in front of the rules; log-probs, alternatives and scores are those of the constrained
        distribution.  None or an empty list: the call without it.  ValueError: a list for another vocabulary, a phrase id
        from <eot> on or in suppress_tokens, a first id that suppress_blank forbids, no_repeat_ngram_size > 0,
        min_new_tokens > 0."""
        if asynchronous or return_logits_vocab:
            raise ValueError("asynchronous / return_logits_vocab are not supported (unused by faster-whisper)")
        boost_h, constraint_h = BoostList._handle_of(boost), ConstraintList._handle_of(constraint)
        top_k, top_p = int(top_k), float(top_p)
        n_alt = int(return_alternatives)
        if not 0 <= n_alt <= MAX_ALTERNATIVES:
            raise ValueError(f"return_alternatives must lie in [0, {MAX_ALTERNATIVES}] (got {return_alternatives})")
        return_token_logprobs = bool(return_token_logprobs) or n_alt > 0
        enc = self._as_encoded(features)
        if len(prompts) != enc._shape[0]:
            raise ValueError(f"got {len(prompts)} prompts for a batch of {enc._shape[0]}")
        if any(len(p) == 0 for p in prompts):
            raise ValueError("prompts must not be empty")
        o = _lib.FwGenOpts()
        o.beam_size, o.patience, o.num_hypotheses = int(beam_size), float(patience), int(num_hypotheses)
        o.length_penalty, o.repetition_penalty = float(length_penalty), float(repetition_penalty)
        o.no_repeat_ngram_size, o.max_length = int(no_repeat_ngram_size), int(max_length)
        o.return_scores, o.return_no_speech_prob = int(return_scores), int(return_no_speech_prob)
        o.max_initial_timestamp_index, o.suppress_blank = int(max_initial_timestamp_index), int(suppress_blank)
        sup = np.asarray([t for t in (suppress_tokens or []) if t >= 0], dtype=np.int32)
        o.suppress_tokens = _lib.as_i32p(sup) if sup.size else None
        o.n_suppress_tokens = int(sup.size)
        o.sampling_topk, o.sampling_temperature = int(sampling_topk), float(sampling_temperature)
        o.min_new_tokens = int(min_new_tokens)
        nh = max(1, int(num_hypotheses))
        ml = max(1, int(max_length))

        def one_call(enc, prompts):
            """one engine call: an encoder output of at most max_batch chunks"""
            B = enc._shape[0]
            flat, offs = _ragged([np.asarray(p, dtype=np.int32) for p in prompts], np.int32, np.int32)
            # CTranslate2 draws from a global generator that advances from call to call; here every engine call gets a
            # seed of its own from a per-model counter (explicit seeds reproduce a call exactly)
            o.seed = int(call_seed(next(self._seed_counter)) if seed is None else seed)
            ids = np.zeros((B, nh, ml), dtype=np.int32)
            lens = np.zeros((B, nh), dtype=np.int32)
            scores = np.zeros((B, nh), dtype=np.float32)
            nsp = np.zeros((B,), dtype=np.float32)
            tlp = elp = aid = alp = eid = elps = None
            if return_token_logprobs:
                tlp = np.zeros((B, nh, ml), dtype=np.float32)
                elp = np.zeros((B, nh), dtype=np.float32)
            if n_alt:
                aid = np.zeros((B, nh, ml, n_alt), dtype=np.int32)
                alp = np.zeros((B, nh, ml, n_alt), dtype=np.float32)
                eid = np.zeros((B, nh, n_alt), dtype=np.int32)
                elps = np.zeros((B, nh, n_alt), dtype=np.float32)
            def f32(a): return _lib.as_f32p(a) if a is not None else None
            def i32(a): return _lib.as_i32p(a) if a is not None else None
            entry, args = _generate_call(
                self._lib, (enc._owner.handle, enc._handle, _lib.as_i32p(flat), _lib.as_i32p(offs), B, C.byref(o)),
                (_lib.as_i32p(ids), _lib.as_i32p(lens), _lib.as_f32p(scores), _lib.as_f32p(nsp)), (f32(tlp), f32(elp)),
                (i32(aid), f32(alp), i32(eid), f32(elps)), n_alt, top_k, top_p, boost_h, constraint_h)
            _lib.check(entry(*args))
            out = []
            for b in range(B):
                seqs = [ids[b, h, :lens[b, h]].tolist() for h in range(nh)]
                sc = [float(scores[b, h]) for h in range(nh)] if return_scores else []
                res = WhisperGenerationResult(seqs, sc, float(nsp[b]) if return_no_speech_prob else 0.0)
                if return_token_logprobs:
                    res.token_logprobs = [tlp[b, h, :lens[b, h]].tolist() for h in range(nh)]
                    res.end_logprobs = [float(elp[b, h]) for h in range(nh)]
                if n_alt:
                    res.token_alternatives = [          # (one tolist per hypothesis, not one per position)
                        [list(zip(i, v)) for i, v in zip(aid[b, h, :lens[b, h]].tolist(), alp[b, h, :lens[b, h]].tolist())]
                        for h in range(nh)]
                    # (id -1: no closing step — the hypothesis was cut at the budget, or the slot holds no hypothesis)
                    res.end_alternatives = [
                        list(zip(eid[b, h].tolist(), elps[b, h].tolist())) if eid[b, h, 0] >= 0 else None
                        for h in range(nh)]
                out.append(res)
            return out
        return self._over_parts(enc, one_call, prompts)

    # ---- detect_language ----------------------------------------------------------------
    def detect_language(self, features: StorageView) -> List[List[Tuple[str, float]]]:
        if not self.is_multilingual:
            raise RuntimeError("detect_language can only be called on multilingual models")
        names = language_token_strings(self._cfg)

        def one_call(enc):
            B, nl = enc._shape[0], self._cfg.n_langs
            ids = np.zeros((B, nl), dtype=np.int32)
            probs = np.zeros((B, nl), dtype=np.float32)
            _lib.check(self._lib.fw_detect_language(enc._owner.handle, enc._handle, B, _lib.as_i32p(ids),
                                                    _lib.as_f32p(probs)))
            return [[(names[int(t) - self._cfg.lang_begin], float(p)) for t, p in zip(ids[b], probs[b])]
                    for b in range(B)]
        return self._over_parts(self._as_encoded(features), one_call)

    # ---- align --------------------------------------------------------------------------
    def align(self, features: StorageView, start_sequence: Sequence[int], text_tokens: List[List[int]],
              num_frames: Union[int, Sequence[int]], *, median_filter_width: int = 7
              ) -> List[WhisperAlignmentResult]:
        enc = self._as_encoded(features)
        if len(text_tokens) != enc._shape[0]:
            raise ValueError(f"got {len(text_tokens)} token lists for a batch of {enc._shape[0]}")
        num_frames = np.asarray([num_frames] * enc._shape[0] if isinstance(num_frames, int) else list(num_frames),
                                dtype=np.int32)
        if num_frames.shape[0] != enc._shape[0]:
            raise ValueError("num_frames must be an int or have one entry per batch item")
        start = np.asarray(list(start_sequence), dtype=np.int32)

        def one_call(enc, text_tokens, nf):
            B = enc._shape[0]
            flat, offs = _ragged([np.asarray(t, dtype=np.int32) for t in text_tokens], np.int32, np.int32)
            max_pairs = int(max((len(t) for t in text_tokens), default=0)) + self._cfg.n_audio_ctx + 2
            pairs = np.zeros((B, max_pairs, 2), dtype=np.int32)
            npairs = np.zeros((B,), dtype=np.int32)
            probs = np.zeros((max(1, flat.shape[0]),), dtype=np.float32)
            _lib.check(self._lib.fw_align(enc._owner.handle, enc._handle, _lib.as_i32p(start), start.shape[0],
                                          _lib.as_i32p(flat), _lib.as_i32p(offs), _lib.as_i32p(nf), B,
                                          int(median_filter_width), max_pairs, _lib.as_i32p(pairs),
                                          _lib.as_i32p(npairs), _lib.as_f32p(probs)))
            return [WhisperAlignmentResult([(int(a), int(t)) for a, t in pairs[b, :npairs[b]]],
                                           probs[offs[b]:offs[b + 1]].tolist()) for b in range(B)]
        return self._over_parts(enc, one_call, text_tokens, num_frames)

    # ---- score --------------------------------------------------------------------------
    _RULE_DEFAULTS = dict(repetition_penalty=1, no_repeat_ngram_size=0, suppress_blank=True, suppress_tokens=(-1,),
                          max_initial_timestamp_index=50)

    def score(self, features: StorageView, prompts: List[List[int]], targets, *, rules: bool = False,
              boost: Optional[BoostList] = None, constraint: Optional[ConstraintList] = None,
              **rule_kwargs) -> List[WhisperScoringResult]:
        """Teacher-forced log-probs of given transcripts (fwamd.h: fw_score; not in CTranslate2's Whisper class).
        targets[b]: one sequence of ids, or a list of up to max_beam_size sequences, scored against chunk b.
        rules=False: the raw distribution.  rules=True: the distribution generate()'s search ranks by, with generate's
        rule keywords and their defaults (repetition_penalty, no_repeat_ngram_size, suppress_blank, suppress_tokens,
        max_initial_timestamp_index); the timestamp rules follow the prompt.  result.score(h, length_penalty=1) is then
        what generate(return_scores=True) reports for the same ids.
        boost: the BoostList of a generate(boost=...) call, added in front of the rules with the sequence's own prefix as the
        generated history; needs rules=True.
        constraint: the ConstraintList of a generate(constraint=...) call, applied behind the boost and in front of the
        rules; needs rules=True.  A target that leaves the list scores -inf from there on."""
        unknown = set(rule_kwargs) - set(self._RULE_DEFAULTS)
        if unknown:
            raise TypeError(f"score() got unexpected keyword arguments {sorted(unknown)}")
        if rule_kwargs and not rules:
            raise ValueError(f"{sorted(rule_kwargs)} need rules=True: without it the raw distribution is scored")
        boost_h, constraint_h = BoostList._handle_of(boost), ConstraintList._handle_of(constraint)
        if boost_h is not None and not rules:
            raise ValueError("boost needs rules=True: the boost is the first step of the decoding rules")
        if constraint_h is not None and not rules:
            raise ValueError("constraint needs rules=True: the constraint is a step of the decoding rules")
        enc = self._as_encoded(features)
        if len(prompts) != enc._shape[0] or len(targets) != enc._shape[0]:
            raise ValueError(f"got {len(prompts)} prompts and {len(targets)} targets for a batch of {enc._shape[0]}")
        if any(len(p) == 0 for p in prompts):
            raise ValueError("prompts must not be empty")

        def candidates(t):   # one sequence of ids -> [sequence]
            t = list(t)
            return [list(s) for s in t] if t and isinstance(t[0], (list, tuple, np.ndarray)) else [t]
        cands = [candidates(t) for t in targets]
        H = max(len(c) for c in cands)
        if H < 1 or H > self._max_beam:
            raise ValueError(f"{H} candidate sequences for one chunk: score() takes 1 .. max_beam_size={self._max_beam}")
        o = None
        if rules:
            kw = dict(self._RULE_DEFAULTS, **rule_kwargs)
            o = _lib.FwGenOpts()
            o.repetition_penalty, o.no_repeat_ngram_size = float(kw["repetition_penalty"]), int(kw["no_repeat_ngram_size"])
            o.max_initial_timestamp_index, o.suppress_blank = int(kw["max_initial_timestamp_index"]), int(kw["suppress_blank"])
            sup = np.asarray([t for t in (kw["suppress_tokens"] or []) if t >= 0], dtype=np.int32)
            o.suppress_tokens = _lib.as_i32p(sup) if sup.size else None
            o.n_suppress_tokens = int(sup.size)

        def one_call(enc, prompts, cands):
            B = enc._shape[0]
            # every chunk gets H rows: a chunk with fewer candidates is filled up with empty sequences, dropped below
            seqs = [c[h] if h < len(c) else [] for c in cands for h in range(H)]
            pflat, poffs = _ragged([np.asarray(p, dtype=np.int32) for p in prompts], np.int32, np.int32)
            tflat, toffs = _ragged([np.asarray(s, dtype=np.int32) for s in seqs], np.int32, np.int32)
            n_out = int(toffs[-1]) + B * H
            lp = np.zeros((n_out,), dtype=np.float32)
            bid = np.zeros((n_out,), dtype=np.int32)
            blp = np.zeros((n_out,), dtype=np.float32)
            head = (enc._owner.handle, enc._handle, _lib.as_i32p(pflat), _lib.as_i32p(poffs), _lib.as_i32p(tflat),
                    _lib.as_i32p(toffs), B, H, C.byref(o) if o is not None else None)
            outs = (_lib.as_f32p(lp), _lib.as_i32p(bid), _lib.as_f32p(blp))
            entry, args = _score_call(self._lib, head, outs, boost_h, constraint_h)
            _lib.check(entry(*args))
            out = []
            for b in range(B):
                res = WhisperScoringResult([], [], [], [], [])
                for h in range(len(cands[b])):
                    i = b * H + h
                    n, e0 = len(seqs[i]), int(toffs[i]) + i
                    res.sequences_ids.append([int(t) for t in seqs[i]])
                    res.token_logprobs.append(lp[e0:e0 + n].tolist())
                    res.end_logprobs.append(float(lp[e0 + n]))
                    res.best_ids.append(bid[e0:e0 + n + 1].tolist())
                    res.best_logprobs.append(blp[e0:e0 + n + 1].tolist())
                out.append(res)
            return out
        return self._over_parts(enc, one_call, prompts, cands)

    # ---- measurement --------------------------------------------------------------------
    def _primary_of(self, replica: int) -> int:
        """index of the replica that owns the decode workspace of `replica`'s device (the first one of the device)"""
        dev = self._replicas[replica].device_index
        return next(i for i, r in enumerate(self._replicas) if r.device_index == dev)

    def profile(self, enable: bool = True, replica: Optional[int] = 0):
        """per-kernel-family HIP-event timing.  replica=None: every worker.  Decode-side families are recorded by
        the replica that owns the device's decode workspace, so that one is switched along."""
        idx = range(len(self._replicas)) if replica is None else sorted({replica, self._primary_of(replica)})
        for i in idx:
            self._lib.fw_prof_enable(self._replicas[i].handle, int(enable))
            self._lib.fw_prof_reset(self._replicas[i].handle)

    def profile_report(self, replica: Optional[int] = 0) -> Dict[str, dict]:
        out = {}
        idx = range(len(self._replicas)) if replica is None else sorted({replica, self._primary_of(replica)})
        for r in idx:
            h = self._replicas[r].handle
            for i in range(self._lib.fw_prof_count()):
                ms, n, fl, by = C.c_double(), C.c_int64(), C.c_double(), C.c_double()
                _lib.check(self._lib.fw_prof_get(h, i, C.byref(ms), C.byref(n), C.byref(fl), C.byref(by)))
                acc = out.setdefault(self._lib.fw_prof_name(i).decode(), dict(ms=0.0, launches=0, flops=0.0, bytes=0.0))
                acc["ms"] += ms.value
                acc["launches"] += n.value
                acc["flops"] += fl.value
                acc["bytes"] += by.value
        return out

    def unload_model(self):
        for r in reversed(self._replicas):     # workers before the replica whose decoder / weights they share
            r.close()

    def __del__(self):
        try:
            self.unload_model()
        except Exception:
            pass


_LANG_CODES = (
    "en zh de es ru ko fr ja pt tr pl ca nl ar sv it id hi fi vi he uk el ms cs ro da hu ta no th ur hr bg lt la mi "
    "ml cy sk te fa lv bn sr az sl kn et mk br eu is hy ne mn bs kk sq sw gl mr pa si km sn yo so af oc ka be tg sd "
    "gu am yi lo uz fo ht ps tk nn mt sa lb my bo tl mg as tt haw ln ha ba jw su yue").split()


def language_token_strings(cfg: WhisperConfig) -> List[str]:
    """'<|en|>' ... in vocabulary order (the reference strips the markers, transcribe.py:1826)."""
    codes = _LANG_CODES[:cfg.n_langs] if cfg.n_langs <= len(_LANG_CODES) else \
        _LANG_CODES + [f"l{i}" for i in range(len(_LANG_CODES), cfg.n_langs)]
    return [f"<|{c}|>" for c in codes]


def _ragged(seqs, dtype, off_dtype=np.int64):
    offs = np.zeros(len(seqs) + 1, dtype=off_dtype)
    for i, s in enumerate(seqs):
        offs[i + 1] = offs[i] + len(s)
    flat = np.zeros(max(1, int(offs[-1])), dtype=dtype)
    for i, s in enumerate(seqs):
        flat[offs[i]:offs[i + 1]] = np.asarray(s, dtype=dtype)
    return flat, offs
