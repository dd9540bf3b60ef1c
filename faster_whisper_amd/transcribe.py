"""Host-side mirror of the reference's batched transcription API for the hot path.

Mirrors (same names, argument meaning, defaults and error behaviour)
    faster_whisper/transcribe.py : Word, Segment, TranscriptionOptions, TranscriptionInfo (:31-108),
        BatchedInferencePipeline.forward / generate_segment_batched / transcribe /
        _batched_segments_generator (:111-617), WhisperModel.__init__ attributes (:620-722),
        encode (:1391-1400), get_prompt (:1532-1565), _split_segments_by_timestamps (:1024-1101),
        find_alignment (:1698-1766), detect_language (:1768-1841), get_suppressed_tokens (:1884-1907),
        get_compression_ratio (:1879-1881)
    faster_whisper/audio.py : pad_or_trim (:111-123)
    faster_whisper/feature_extractor.py : FeatureExtractor (the arithmetic runs on the GPU here)
but is written for this engine: features are computed on the GPU, the backend is
`faster_whisper_amd.backend.Whisper`, and `transcribe(..., shard=True)` partitions the chunk
list over the ranks of a torch.distributed job.

Also here: the sequential seek loop
(`WhisperModel.transcribe` / `generate_segments` :747-1022, :1103-1389), the temperature-fallback ladder
(`generate_with_fallback` :1402-1530) and word timestamps (`add_word_timestamps` :1567-1696; heuristics in
words.py, speech chunking in vad.py).  The host logic is pinned against the reference's own code driven by a
scripted backend (oracle/gen_golden_host.py -> tests/golden/host_*.json).

Out of scope: the Silero VAD network itself (row f-3: speech probabilities are an input
here) and PyAV decoding (row f-4: audio is a 16 kHz float32 ndarray).
"""
import json
import logging
import os
import zlib
from dataclasses import dataclass, field, fields
from math import ceil
from typing import Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np

from .backend import StorageView, Whisper, attempt_seed, language_token_strings, recording_seed
from .config import WhisperConfig

_LOG = logging.getLogger("faster_whisper")


def _resample_device_index(backend) -> Optional[int]:
    """decode_audio's device_index for a transcribe(path) call: with FWAMD_RESAMPLE_DEVICE=1 in the environment file audio
    is rate-converted on the model's (first) GPU (audio.resample_device: the same samples as the numpy filter); unset, on
    the host"""
    if os.environ.get("FWAMD_RESAMPLE_DEVICE") != "1":
        return None
    idx = backend.device_index
    return idx if isinstance(idx, int) else idx[0]


@dataclass
class Word:
    start: float
    end: float
    word: str
    probability: float


@dataclass
class Segment:
    id: int
    seek: int
    start: float
    end: float
    text: str
    tokens: List[int]
    avg_logprob: float
    compression_ratio: float
    no_speech_prob: float
    words: Optional[List[Word]]
    temperature: Optional[float]


@dataclass
class ScoredSegment(Segment):
    """what transcribe(token_logprobs=True) yields: a Segment plus token_logprobs[i] = the log-prob of tokens[i] (timestamp
    tokens included) under the distribution the decoder chose from, i.e. after the logits rules"""
    token_logprobs: List[float]


@dataclass
class AlternativesSegment(ScoredSegment):
    """what transcribe(token_alternatives=N) yields: a ScoredSegment plus token_alternatives[i] = the N most likely
    (id, log-prob) pairs of the distribution tokens[i] was chosen from, log-prob descending then id ascending ((0, -inf)
    where the rules left fewer than N ids)"""
    token_alternatives: List[List[Tuple[int, float]]]


def _slice_token_logprobs(subs: List[dict], logprobs: List[float], key: str = "token_logprobs") -> None:
    """gives every sub-segment dict of one chunk the log-probs of its tokens: _split_segments_by_timestamps cuts
    consecutive slices of the chunk's tokens from index 0 on (what follows the last cut belongs to no sub-segment).
    key="token_alternatives": the same cut of the chunk's per-token alternatives."""
    pos = 0
    for s in subs:
        s[key] = list(logprobs[pos:pos + len(s["tokens"])])
        pos += len(s["tokens"])


def _slice_token_values(subs: List[dict], logprobs: List[float], alternatives: Optional[list] = None) -> None:
    """the per-token values a token_logprobs / token_alternatives call attaches to the sub-segments of one chunk"""
    _slice_token_logprobs(subs, logprobs)
    if alternatives is not None:
        _slice_token_logprobs(subs, alternatives, "token_alternatives")


def _check_trunc_arguments(sampling_top_k, sampling_top_p) -> None:
    """sampling_top_k: an integer >= 0; sampling_top_p: a number in (0, 1] (ValueError) — what fw_generate_trunc accepts,
    checked before anything is decoded"""
    if isinstance(sampling_top_k, bool) or not isinstance(sampling_top_k, (int, np.integer)) or sampling_top_k < 0:
        raise ValueError(f"sampling_top_k must be an integer >= 0 (got {sampling_top_k!r})")
    if isinstance(sampling_top_p, bool) or not isinstance(sampling_top_p, (int, float, np.integer, np.floating)) \
            or not 0 < sampling_top_p <= 1:
        raise ValueError(f"sampling_top_p must lie in (0, 1] (got {sampling_top_p!r})")


@dataclass
class TranscriptionOptions:
    beam_size: int
    best_of: int
    patience: float
    length_penalty: float
    repetition_penalty: float
    no_repeat_ngram_size: int
    log_prob_threshold: Optional[float]
    no_speech_threshold: Optional[float]
    compression_ratio_threshold: Optional[float]
    condition_on_previous_text: bool
    prompt_reset_on_temperature: float
    temperatures: List[float]
    initial_prompt: Optional[Union[str, Iterable[int]]]
    prefix: Optional[str]
    suppress_blank: bool
    suppress_tokens: Optional[List[int]]
    without_timestamps: bool
    max_initial_timestamp: float
    word_timestamps: bool
    prepend_punctuations: str
    append_punctuations: str
    multilingual: bool
    max_new_tokens: Optional[int]
    clip_timestamps: Union[str, List[float]]
    hallucination_silence_threshold: Optional[float]
    hotwords: Optional[str]


@dataclass
class TranscriptionInfo:
    language: str
    language_probability: float
    duration: float
    duration_after_vad: float
    all_language_probs: Optional[List[Tuple[str, float]]]
    transcription_options: TranscriptionOptions
    vad_options: object


def _transcription_options(args, tokenizer: "Tokenizer", **derived) -> TranscriptionOptions:
    """The TranscriptionOptions of a transcribe() call.  args: the call's arguments by name.  Every field takes the
    argument of its own name unless `derived` gives its value (`temperatures`, and whatever the driver fixes or has
    resolved); a non-empty suppress_tokens is expanded by get_suppressed_tokens."""
    values = {**args, **derived}
    if values["suppress_tokens"]:
        values["suppress_tokens"] = get_suppressed_tokens(tokenizer, values["suppress_tokens"])
    return TranscriptionOptions(**{f.name: values[f.name] for f in fields(TranscriptionOptions)})


def _check_boost_arguments(boost_phrases, phrase_boost) -> None:
    """boost_phrases: None, or a sequence of strings; with phrases phrase_boost must be given (ValueError)"""
    if boost_phrases is None:
        return
    if isinstance(boost_phrases, (str, bytes)) or not all(isinstance(p, str) for p in boost_phrases):
        raise ValueError("boost_phrases must be a sequence of strings, one per phrase")
    if len(boost_phrases) and phrase_boost is None:
        raise ValueError("boost_phrases need phrase_boost: the strength of the boost in logit units has no default")


def _check_constraint_arguments(allowed_phrases) -> None:
    """allowed_phrases: None, or a sequence of strings (ValueError)"""
    if allowed_phrases is None:
        return
    if isinstance(allowed_phrases, (str, bytes)) or not all(isinstance(p, str) for p in allowed_phrases):
        raise ValueError("allowed_phrases must be a sequence of strings, one per phrase")


@dataclass(frozen=True)
class DecodeExtras:
    """What a transcription call asks of its decodes beyond the reference's options, carried as ONE value from the entry
    point to model.generate.  boost / constraint: the call's built lists (boost_list_for / constraint_list_for), the same
    objects for every window, attempt, batch and recording."""
    token_logprobs: bool = False
    token_alternatives: int = 0
    boost: object = None
    constraint: object = None
    sampling_top_k: int = 0
    sampling_top_p: float = 1.0

    def generate_keywords(self, sampled: bool = False) -> dict:
        """the keywords of model.generate — only those that are set, so that a backend that does not know them (a scripted
        backend, CTranslate2 behind the shim) never sees them otherwise.  sampled: a rung with temperature > 0, the only
        kind of decode the sampling limits apply to."""
        kw = {}
        if self.token_alternatives:
            kw["return_alternatives"] = int(self.token_alternatives)
        elif self.token_logprobs:
            kw["return_token_logprobs"] = True
        if self.boost is not None:
            kw["boost"] = self.boost
        if self.constraint is not None:
            kw["constraint"] = self.constraint
        if sampled and self.sampling_top_k:
            kw["top_k"] = int(self.sampling_top_k)
        if sampled and self.sampling_top_p != 1:
            kw["top_p"] = float(self.sampling_top_p)
        return kw

    def keyword(self) -> dict:
        """the keyword of an internal boundary — none when nothing is set (as generate_keywords)"""
        return {} if self == DecodeExtras() else {"extras": self}


def _decode_extras(model: "WhisperModel", a) -> DecodeExtras:
    """The DecodeExtras of an entry point's arguments `a` (by name), checked before anything is loaded or decoded
    (ValueError).  The lists are built here, once per call: the text encoding of a phrase does not depend on task or
    language, so any tokenizer of the model gives the same ids."""
    _check_boost_arguments(a["boost_phrases"], a["phrase_boost"])
    _check_constraint_arguments(a["allowed_phrases"])
    _check_trunc_arguments(a["sampling_top_k"], a["sampling_top_p"])
    tokenizer = model.make_tokenizer() if a["boost_phrases"] or a["allowed_phrases"] else None
    return DecodeExtras(token_logprobs=a["token_logprobs"], token_alternatives=a["token_alternatives"],
                        boost=model.boost_list_for(a["boost_phrases"], a["phrase_boost"], tokenizer),
                        constraint=model.constraint_list_for(a["allowed_phrases"], tokenizer),
                        sampling_top_k=a["sampling_top_k"], sampling_top_p=a["sampling_top_p"])


def _per_recording(value, n, name, is_single):
    """one value for all recordings, or a sequence with one entry per recording -> a list of n"""
    if is_single(value):
        return [value] * n
    value = list(value)
    if len(value) != n:
        raise ValueError(f"{name} has {len(value)} entries for {n} recordings")
    return value


def _avg_logprob(result, length_penalty: float) -> float:
    """average log-prob per token (the closing <eot> counted) of a generate() result's first hypothesis: its score with
    the length normalisation undone (transcribe.py:241-246, :1462-1467)"""
    n = len(result.sequences_ids[0])
    return result.scores[0] * (n ** length_penalty) / (n + 1)


def _make_segment(values: dict, token_logprobs: Optional[List[float]] = None,
                  token_alternatives: Optional[list] = None) -> Segment:
    """a Segment, or with token_logprobs (what a token_logprobs=True call attaches to its sub-segments) a ScoredSegment,
    or with token_alternatives as well (a token_alternatives=N call) an AlternativesSegment"""
    if token_logprobs is None:
        return Segment(**values)
    if token_alternatives is None:
        return ScoredSegment(token_logprobs=token_logprobs, **values)
    return AlternativesSegment(token_logprobs=token_logprobs, token_alternatives=token_alternatives, **values)


def pad_or_trim(array: np.ndarray, length: int = 3000, *, axis: int = -1) -> np.ndarray:
    """trim to `length` frames or right-pad with zeros (audio.py:111-123)"""
    if array.shape[axis] > length:
        array = np.take(array, np.arange(length), axis=axis)
    if array.shape[axis] < length:
        pad = [(0, 0)] * array.ndim
        pad[axis] = (0, length - array.shape[axis])
        array = np.pad(array, pad)
    return array


def get_compression_ratio(text: str) -> float:
    raw = text.encode("utf-8")
    return len(raw) / len(zlib.compress(raw))


class FeatureExtractor:
    """Same constructor / call signature as the reference's numpy FeatureExtractor; the
    arithmetic runs in the HIP log-mel kernel of the model it is attached to."""

    def __init__(self, feature_size=80, sampling_rate=16000, hop_length=160, chunk_length=30, n_fft=400,
                 backend: Optional[Whisper] = None):
        if (sampling_rate, hop_length, n_fft) != (16000, 160, 400):
            raise ValueError("the HIP log-mel kernel is built for sampling_rate=16000, hop_length=160, n_fft=400")
        self.n_fft, self.hop_length, self.chunk_length = n_fft, hop_length, chunk_length
        self.n_samples = chunk_length * sampling_rate
        self.nb_max_frames = self.n_samples // hop_length
        self.time_per_frame = hop_length / sampling_rate
        self.sampling_rate = sampling_rate
        self.feature_size = feature_size
        self._backend = backend

    def __call__(self, waveform: np.ndarray, padding=160, chunk_length=None) -> np.ndarray:
        if self._backend is None:
            raise RuntimeError("FeatureExtractor is not attached to a GPU model (no CPU implementation)")
        if padding != 160:
            raise ValueError("only padding=160 (the reference default) is supported")
        if chunk_length is not None:
            self.n_samples = chunk_length * self.sampling_rate
            self.nb_max_frames = self.n_samples // self.hop_length
        return self._backend.log_mel_full(np.asarray(waveform, dtype=np.float32))


class Tokenizer:
    """Special-token view of the Whisper vocabulary (tokenizer.py:9-112).  Text encode/decode
    is delegated to a HF `tokenizers.Tokenizer` when a tokenizer.json is available; without
    one (synthetic weights) ids are rendered as `<id>` so the pipeline still runs end to end."""

    def __init__(self, hf_tokenizer, cfg: WhisperConfig, multilingual: bool, task: Optional[str] = None,
                 language: Optional[str] = None):
        self.tokenizer = hf_tokenizer
        self.cfg = cfg
        self.sot, self.eot = cfg.sot, cfg.eot
        self.sot_prev, self.sot_lm = cfg.sot_prev, cfg.sot_lm
        self.no_speech, self.no_timestamps = cfg.no_speech, cfg.no_timestamps
        self.transcribe, self.translate = cfg.transcribe, cfg.translate
        self.timestamp_begin = cfg.timestamp_begin
        if multilingual:
            if task not in ("transcribe", "translate"):
                raise ValueError(f"'{task}' is not a valid task (accepted tasks: transcribe, translate)")
            names = [s[2:-2] for s in language_token_strings(cfg)]
            if language not in names:
                raise ValueError(f"'{language}' is not a valid language code")
            self.task = cfg.transcribe if task == "transcribe" else cfg.translate
            self.language = cfg.lang_begin + names.index(language)
            self.language_code = language
        else:
            self.task = None
            self.language = None
            self.language_code = "en"

    @property
    def sot_sequence(self) -> List[int]:
        seq = [self.sot]
        if self.language is not None:
            seq.append(self.language)
        if self.task is not None:
            seq.append(self.task)
        return seq

    @property
    def non_speech_tokens(self) -> Tuple[int, ...]:
        # needs the real vocabulary (tokenizer.py:114-148); empty for synthetic models
        if self.tokenizer is None:
            return ()
        symbols = list('"#()*+/:;<=>@[\\]^_`{|}~「」『』') + "<< >> <<< >>> -- --- -( -[ (' (\" (( )) ((( ))) [[ ]] {{ }} ♪♪ ♪♪♪".split()
        miscellaneous = set("♩♪♫♬♭♮♯")
        result = {self.encode(" -")[0], self.encode(" '")[0]}
        for symbol in symbols + list(miscellaneous):
            for tokens in (self.encode(symbol), self.encode(" " + symbol)):
                if len(tokens) == 1 or symbol in miscellaneous:
                    result.add(tokens[0])
        return tuple(sorted(result))

    def encode(self, text: str) -> List[int]:
        if self.tokenizer is None:
            raise RuntimeError("text prompts need a tokenizer.json (this model has none)")
        return self.tokenizer.encode(text, add_special_tokens=False).ids

    def decode(self, tokens: List[int]) -> str:
        text_tokens = [t for t in tokens if t < self.eot]
        return self._render(text_tokens)

    def _render(self, ids: List[int]) -> str:
        """text of a run of non-timestamp ids (special tokens are dropped, as HF `decode` does)"""
        if self.tokenizer is None:
            return "".join(f"<{t}>" for t in ids if t < self.eot)
        return self.tokenizer.decode(ids)

    def decode_with_timestamps(self, tokens: List[int]) -> str:
        """text with every timestamp token rendered as <|s.ss|> (tokenizer.py:95-112)"""
        out, run = [], []
        for t in tokens:
            if t >= self.timestamp_begin:
                out.append(self._render(run))
                out.append(f"<|{(t - self.timestamp_begin) * 0.02:.2f}|>")
                run = []
            else:
                run.append(t)
        out.append(self._render(run))
        return "".join(out)

    # ---- word splitting (tokenizer.py:150-208) -------------------------------------------
    def split_to_word_tokens(self, tokens: List[int]) -> Tuple[List[str], List[List[int]]]:
        # languages written without spaces are split wherever the bytes so far decode to whole characters
        if self.language_code in {"zh", "ja", "th", "lo", "my", "yue"}:
            return self.split_tokens_on_unicode(tokens)
        return self.split_tokens_on_spaces(tokens)

    def split_tokens_on_unicode(self, tokens: List[int]) -> Tuple[List[str], List[List[int]]]:
        """groups tokens until they decode without a dangling partial UTF-8 sequence (U+FFFD), unless the
        full text really has U+FFFD at that position"""
        full = self.decode_with_timestamps(tokens)
        words, groups, pending, consumed = [], [], [], 0
        for t in tokens:
            pending.append(t)
            text = self.decode_with_timestamps(pending)
            bad = text.find("�")
            if bad < 0 or (consumed + bad < len(full) and full[consumed + bad] == "�"):
                words.append(text)
                groups.append(pending)
                consumed += len(text)
                pending = []
        return words, groups

    def split_tokens_on_spaces(self, tokens: List[int]) -> Tuple[List[str], List[List[int]]]:
        """unicode pieces are joined into words: a piece opens a new word when it is a special token, starts
        with a space, is a lone punctuation mark, or is the very first piece"""
        import string
        words: List[str] = []
        groups: List[List[int]] = []
        for piece, ids in zip(*self.split_tokens_on_unicode(tokens)):
            opens = (ids[0] >= self.eot or piece.startswith(" ") or piece.strip() in string.punctuation
                     or not words)
            if opens:
                words.append(piece)
                groups.append(ids)
            else:
                words[-1] += piece
                groups[-1].extend(ids)
        return words, groups


def get_suppressed_tokens(tokenizer: Tokenizer, suppress_tokens) -> Optional[Tuple[int, ...]]:
    """suppress set = user ids (-1 expands to the non-speech tokens) + task/sot/no_speech specials,
    sorted tuple (transcribe.py:1884-1907)"""
    if -1 in suppress_tokens:
        suppress_tokens = [t for t in suppress_tokens if t >= 0]
        suppress_tokens.extend(tokenizer.non_speech_tokens)
    elif suppress_tokens is None or len(suppress_tokens) == 0:
        suppress_tokens = []
    else:
        assert isinstance(suppress_tokens, list), "suppress_tokens must be a list"
        suppress_tokens = list(suppress_tokens)
    suppress_tokens.extend([tokenizer.transcribe, tokenizer.translate, tokenizer.sot, tokenizer.sot_prev,
                            tokenizer.sot_lm, tokenizer.no_speech])
    return tuple(sorted(set(suppress_tokens)))


class WhisperModel:
    """Model + the helpers the batched pipeline needs (reference: WhisperModel.__init__ :620-722)."""

    def __init__(self, model_size_or_path: str, device: str = "auto", device_index: Union[int, List[int]] = 0,
                 compute_type: str = "default", cpu_threads: int = 0, num_workers: int = 1,
                 download_root: Optional[str] = None, local_files_only: bool = False, files: dict = None,
                 revision: Optional[str] = None, use_auth_token=None, **model_kwargs):
        self.logger = _LOG
        tokenizer_bytes = preprocessor_bytes = None
        if files:
            files = dict(files)
            tokenizer_bytes = files.pop("tokenizer.json", None)
            preprocessor_bytes = files.pop("preprocessor_config.json", None)
        model_path = model_size_or_path
        self.model = Whisper(model_path, device=device, device_index=device_index, compute_type=compute_type,
                             intra_threads=cpu_threads, inter_threads=num_workers, files=files, **model_kwargs)
        cfg = self.model.config
        self.hf_tokenizer = None
        tok_file = os.path.join(model_path, "tokenizer.json") if isinstance(model_path, str) else ""
        if tokenizer_bytes or os.path.isfile(tok_file):
            import tokenizers
            self.hf_tokenizer = (tokenizers.Tokenizer.from_buffer(tokenizer_bytes) if tokenizer_bytes
                                 else tokenizers.Tokenizer.from_file(tok_file))
        self.feat_kwargs = self._get_feature_kwargs(model_path, preprocessor_bytes)
        self.feat_kwargs.setdefault("feature_size", cfg.n_mels)
        self.feature_extractor = FeatureExtractor(**self.feat_kwargs, backend=self.model)
        self.input_stride = 2
        self.num_samples_per_token = self.feature_extractor.hop_length * self.input_stride
        self.frames_per_second = self.feature_extractor.sampling_rate // self.feature_extractor.hop_length
        self.tokens_per_second = self.feature_extractor.sampling_rate // self.num_samples_per_token
        self.time_precision = 0.02
        self.max_length = 448

    @property
    def supported_languages(self) -> List[str]:
        if not self.model.is_multilingual:
            return ["en"]
        return [s[2:-2] for s in language_token_strings(self.model.config)]

    def _get_feature_kwargs(self, model_path, preprocessor_bytes=None) -> dict:
        config = {}
        try:
            path = os.path.join(model_path, "preprocessor_config.json") if isinstance(model_path, str) else ""
            if preprocessor_bytes:
                config = json.loads(preprocessor_bytes)
            elif os.path.isfile(path):
                with open(path, "r", encoding="utf-8") as f:
                    config = json.load(f)
            else:
                return config
            valid = ("feature_size", "sampling_rate", "hop_length", "chunk_length", "n_fft")
            return {k: v for k, v in config.items() if k in valid}
        except json.JSONDecodeError as e:
            self.logger.warning("Could not load preprocessor config: %s", e)
        return config

    # ---- what every transcribe entry point decides the same way ----
    def _load_audio(self, audio) -> np.ndarray:
        """a path or file object -> its samples at the model's rate, float32 (WAVE and FLAC natively, other containers
        through PyAV); an array is returned as it is"""
        if isinstance(audio, np.ndarray):
            return audio
        from .audio import decode_audio
        return decode_audio(audio, sampling_rate=self.feature_extractor.sampling_rate,
                            device_index=_resample_device_index(self.model))

    def _effective_multilingual(self, multilingual: bool) -> bool:
        if multilingual and not self.model.is_multilingual:
            self.logger.warning("The current model is English-only but the multilingual parameter is set to"
                                "True; setting to False instead.")
            return False
        return multilingual

    def _effective_language(self, language: str) -> str:
        """the language a call that names `language` decodes in"""
        if not self.model.is_multilingual and language != "en":
            self.logger.warning("The current model is English-only but the language parameter is set to '%s'; "
                                "using 'en' instead." % language)
            return "en"
        return language

    def _max_length_for(self, prompt: List[int], max_new_tokens: Optional[int]) -> int:
        """generate()'s max_length for `prompt`"""
        max_length = len(prompt) + max_new_tokens if max_new_tokens is not None else self.max_length
        if max_length > self.max_length:
            raise ValueError(
                f"The length of the prompt is {len(prompt)}, and the `max_new_tokens` {max_length - len(prompt)}. "
                f"Thus, the combined length of the prompt and `max_new_tokens` is: {max_length}. This exceeds the "
                f"`max_length` of the Whisper model: {self.max_length}. You should either reduce the length of your "
                f"prompt, or reduce the value of `max_new_tokens`, so that their combined length is less that "
                f"{self.max_length}.")
        return max_length

    def _workers(self) -> int:
        """worker replicas of the backend = batches (or recordings) the host drivers may keep in flight"""
        return int(getattr(self.model, "inter_threads", 1) or 1)

    # ---- sequential path (reference transcribe.py:747-1022, :1103-1389) ----
    def transcribe(self, audio: np.ndarray, language: Optional[str] = None, task: str = "transcribe",
                   log_progress: bool = False, beam_size: int = 5, best_of: int = 5, patience: float = 1,
                   length_penalty: float = 1, repetition_penalty: float = 1, no_repeat_ngram_size: int = 0,
                   temperature=(0.0, 0.2, 0.4, 0.6, 0.8, 1.0), compression_ratio_threshold: Optional[float] = 2.4,
                   log_prob_threshold: Optional[float] = -1.0, no_speech_threshold: Optional[float] = 0.6,
                   condition_on_previous_text: bool = True, prompt_reset_on_temperature: float = 0.5,
                   initial_prompt=None, prefix: Optional[str] = None, suppress_blank: bool = True,
                   suppress_tokens: Optional[List[int]] = [-1], without_timestamps: bool = False,
                   max_initial_timestamp: float = 1.0, word_timestamps: bool = False,
                   prepend_punctuations: str = "\"'“¿([{-", append_punctuations: str = "\"'.。,，!！?？:：”)]}、",
                   multilingual: bool = False, vad_filter: bool = False, vad_parameters=None,
                   max_new_tokens: Optional[int] = None, chunk_length: Optional[int] = None,
                   clip_timestamps: Union[str, List[float]] = "0",
                   hallucination_silence_threshold: Optional[float] = None, hotwords: Optional[str] = None,
                   language_detection_threshold: Optional[float] = 0.5, language_detection_segments: int = 1,
                   vad_speech_probs=None, token_logprobs: bool = False, sampling_seed: Optional[int] = None,
                   token_alternatives: int = 0, boost_phrases: Optional[Sequence[str]] = None,
                   phrase_boost: Optional[float] = None, sampling_top_k: int = 0, sampling_top_p: float = 1.0,
                   allowed_phrases: Optional[Sequence[str]] = None):
        """Sequential (seek-loop) transcription: 30 s windows decoded one after the other, each conditioned on
        the text before it, with the temperature-fallback ladder.  Same arguments / defaults / return value
        as the reference's WhisperModel.transcribe; `vad_speech_probs` (not in the reference) feeds
        vad.get_speech_timestamps with precomputed window probabilities instead of running the Silero network.
        token_logprobs=True (not in the reference): every segment is a ScoredSegment, whose token_logprobs are those of
        the decode the fallback ladder kept; every other field is what the call without the keyword yields.
        token_alternatives=N (not in the reference; 1 <= N <= backend.MAX_ALTERNATIVES): every segment is an
        AlternativesSegment, a ScoredSegment whose token_alternatives[i] lists the N most likely (id, log-prob) pairs at
        the position of tokens[i], again those of the decode the ladder kept.
        sampling_seed (not in the reference): makes the sampled attempts of the temperature fallback reproducible.  The
        attempt at rung t of the ladder for the window at frame `seek` samples with backend.attempt_seed(sampling_seed,
        seek, t): the same recording with the same seed gives the same transcript whatever else the model decodes before
        or beside it.  None (the default): every sampling call takes the next seed of the model's call counter.
        boost_phrases, phrase_boost (not in the reference): see boost_list_for — names and terms made more likely by
        phrase_boost at the logit, in every window and every attempt of the fallback ladder, without spending prompt text
        as `hotwords` does.
        sampling_top_k, sampling_top_p (not in the reference): limits on the sampled attempts of the fallback ladder (the
        rungs with temperature > 0; the attempt at temperature 0 is a beam search and takes none): every draw comes from
        the sampling_top_k most likely tokens, then from the nucleus that holds sampling_top_p of their tempered mass
        (include/fwamd.h: fw_generate_trunc).  0 / 1.0 (the defaults): the whole distribution, as the reference samples.
        allowed_phrases (not in the reference): see constraint_list_for — every decoded window is then exactly ONE phrase
        of the list, in every attempt of the fallback ladder.  Composes with boost_phrases."""
        args = dict(locals())               # the call's arguments by name
        return self._transcribe(args, _decode_extras(self, args))

    def _transcribe(self, a: dict, extras: DecodeExtras):
        """transcribe() behind its arguments `a` (by name) and their DecodeExtras (transcribe_many builds ONE for all its
        recordings)"""
        from .vad import VadOptions, collect_chunks, get_speech_timestamps
        from .words import restore_speech_timestamps
        sr = self.feature_extractor.sampling_rate
        multilingual = self._effective_multilingual(a["multilingual"])
        audio = self._load_audio(a["audio"])
        duration = audio.shape[0] / sr
        duration_after_vad = duration
        speech_chunks = None
        vad_parameters, clip_timestamps, language = a["vad_parameters"], a["clip_timestamps"], a["language"]
        if a["vad_filter"] and clip_timestamps == "0":
            if vad_parameters is None:
                vad_parameters = VadOptions()
            elif isinstance(vad_parameters, dict):
                vad_parameters = VadOptions(**vad_parameters)
            speech_chunks = get_speech_timestamps(audio, vad_parameters, speech_probs=a["vad_speech_probs"])
            audio_chunks, _ = collect_chunks(audio, speech_chunks)
            audio = np.concatenate(audio_chunks, axis=0)
            duration_after_vad = audio.shape[0] / sr
        features = self.feature_extractor(audio, chunk_length=a["chunk_length"])

        all_language_probs = None
        if language is None:
            if not self.model.is_multilingual:
                language, language_probability = "en", 1
            else:
                first = float(clip_timestamps.split(",")[0]) if isinstance(clip_timestamps, str) else clip_timestamps[0]
                content_frames = features.shape[-1] - 1
                at = first * self.frames_per_second
                seek = int(at) if at < content_frames else 0
                language, language_probability, all_language_probs = self.detect_language(
                    features=features[..., seek:], language_detection_segments=a["language_detection_segments"],
                    language_detection_threshold=a["language_detection_threshold"])
        else:
            language, language_probability = self._effective_language(language), 1
        tokenizer = self.make_tokenizer(task=a["task"], language=language)
        temperature, sampling_seed = a["temperature"], a["sampling_seed"]
        options = _transcription_options(
            a, tokenizer, multilingual=multilingual,
            temperatures=(temperature if isinstance(temperature, (list, tuple)) else [temperature]))
        segments = self.generate_segments(features, tokenizer, options, a["log_progress"], None, **extras.keyword(),
                                          **(dict(sampling_seed=int(sampling_seed)) if sampling_seed is not None else {}))
        if speech_chunks:
            segments = restore_speech_timestamps(segments, speech_chunks, sr)
        info = TranscriptionInfo(language=language, language_probability=language_probability, duration=duration,
                                 duration_after_vad=duration_after_vad, transcription_options=options,
                                 vad_options=vad_parameters, all_language_probs=all_language_probs)
        return segments, info

    # ---- many recordings through the sequential path ----
    def transcribe_many(self, audios: Sequence[Union[str, np.ndarray]], *, language=None, initial_prompt=None,
                        sampling_seed=None, **transcribe_kwargs) -> List[Tuple[List[Segment], TranscriptionInfo]]:
        """Sequential (seek-loop) transcription of several recordings in ONE call: the sequential counterpart of
        BatchedInferencePipeline.transcribe_many.  result[i] = (list of segments, info) in input order.

        The N transcribe() generators are run to completion on a pool of at most `num_workers` threads; each thread
        works on one worker replica, as concurrent transcribe() calls do.  The windows the threads decode at the same
        time share decode runs — also with condition_on_previous_text=True, where every window's prompt carries a
        different amount of previous text: calls of different prompt lengths may share a run (include/fwamd.h).

        language, initial_prompt: one value for all recordings (None, a string, for initial_prompt also a sequence of
        token ids), or a sequence with one entry per recording.  Every other keyword is transcribe()'s.

        sampling_seed: None, one integer, or a sequence with one integer per recording.  An integer s gives recording i
        the value backend.recording_seed(s, i).

        With a temperature ladder that never leaves 0 (`temperature=0`, or thresholds that no decode fails) result[i] is
        field for field what `transcribe(audios[i], ...)` alone returns: a decode run gives every caller what it gets
        alone.  With sampling_seed that also holds when the fallback samples (temperature > 0): result[i] is field for
        field `transcribe(audios[i], sampling_seed=recording_seed(s, i), ...)`, whatever the thread timing — every
        sampled attempt's seed is a function of (seed of its recording, window, rung) alone, and sampled attempts that
        meet in a decode run (they do: sampling calls share runs among themselves) each draw what they draw alone.
        Without sampling_seed the sampled attempts take their seeds from the model's call counter in arrival order, and
        which recording gets which seed depends on timing.
        boost_phrases / phrase_boost: ONE boost list is built here and handed to every recording's transcription, so the
        windows of different recordings keep sharing decode runs (calls share a run only with an equal list).
        allowed_phrases: likewise ONE constraint list for every recording.
        sampling_top_k / sampling_top_p (not in the reference): transcribe()'s, the same limits for every recording; sampled
        attempts share decode runs whatever their limits.
        An exception in one recording is raised here, after the recordings already started have finished."""
        import inspect
        n = len(audios)
        a = inspect.signature(self.transcribe).bind(None, **transcribe_kwargs)     # transcribe's keywords and defaults
        a.apply_defaults()
        a = a.arguments
        extras = _decode_extras(self, a)
        if n == 0:
            return []
        languages = _per_recording(language, n, "language", lambda v: v is None or isinstance(v, str))
        prompts = _per_recording(
            initial_prompt, n, "initial_prompt",
            lambda v: v is None or isinstance(v, str)
            or (len(v) != 0 and all(isinstance(t, (int, np.integer)) for t in v)))

        if sampling_seed is None:
            seeds = [None] * n
        elif isinstance(sampling_seed, (int, np.integer)):
            seeds = [recording_seed(int(sampling_seed), i) for i in range(n)]
        else:
            seeds = _per_recording(sampling_seed, n, "sampling_seed", lambda v: False)

        def one(i):
            segments, info = self._transcribe(dict(a, audio=audios[i], language=languages[i], initial_prompt=prompts[i],
                                                   sampling_seed=seeds[i]), extras)
            return list(segments), info

        workers = min(n, self._workers())
        if workers <= 1:
            return [one(i) for i in range(n)]
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=workers) as pool:
            futures = [pool.submit(one, i) for i in range(n)]
            return [f.result() for f in futures]

    def generate_segments(self, features: np.ndarray, tokenizer: Tokenizer, options: TranscriptionOptions,
                          log_progress: bool = False, encoder_output: Optional[StorageView] = None,
                          sampling_seed: Optional[int] = None, extras: DecodeExtras = DecodeExtras()):
        """The seek loop (generator of Segment).  For every clip [start, end) of `options.clip_timestamps`
        (frames; an odd count runs to the end of the audio) windows of up to 30 s are decoded at `seek`;
        the timestamps the model emitted (or the last word's end, or a hallucination-silence skip) decide
        where the next window starts."""
        from .words import seek_after_words
        fe = self.feature_extractor
        tpf, fps = fe.time_per_frame, self.frames_per_second
        content_frames = features.shape[-1] - 1
        content_duration = float(content_frames * tpf)
        if isinstance(options.clip_timestamps, str):
            options.clip_timestamps = [float(x) for x in options.clip_timestamps.split(",")] \
                if options.clip_timestamps else []
        marks = [round(t * fps) for t in options.clip_timestamps] or [0]
        if len(marks) % 2 == 1:
            marks.append(content_frames)
        clips = list(zip(marks[::2], marks[1::2]))

        all_tokens: List[int] = []
        prompt_reset_since = 0
        if options.initial_prompt is not None:
            if isinstance(options.initial_prompt, str):
                all_tokens.extend(tokenizer.encode(" " + options.initial_prompt.strip()))
            else:
                all_tokens.extend(options.initial_prompt)
        pbar = None
        if log_progress:
            from tqdm import tqdm
            pbar = tqdm(total=content_duration, unit="seconds")
        idx = 0
        last_speech_timestamp = 0.0
        for clip_start, clip_end in clips:
            clip_end = min(clip_end, content_frames)
            seek = clip_start
            while True:
                seek = max(seek, clip_start)
                if seek >= clip_end:
                    break
                previous_seek = seek
                time_offset = seek * tpf
                window_end_time = float((seek + fe.nb_max_frames) * tpf)
                segment_size = min(fe.nb_max_frames, content_frames - seek, clip_end - seek)
                segment_duration = segment_size * tpf
                window = pad_or_trim(features[:, seek:seek + segment_size])
                previous_tokens = all_tokens[prompt_reset_since:]
                if seek > 0 or encoder_output is None:
                    encoder_output = self.encode(window)
                if options.multilingual:
                    language_token, _ = self.model.detect_language(encoder_output)[0][0]
                    names = language_token_strings(self.model.config)
                    tokenizer.language = self.model.config.lang_begin + names.index(language_token)
                    tokenizer.language_code = language_token[2:-2]
                prompt = self.get_prompt(tokenizer, previous_tokens, without_timestamps=options.without_timestamps,
                                         prefix=options.prefix if seek == 0 else None, hotwords=options.hotwords)
                result, avg_logprob, temperature, compression_ratio = self.generate_with_fallback(
                    encoder_output, prompt, tokenizer, options, **extras.keyword(),
                    **(dict(sampling_seed=sampling_seed, seek=seek) if sampling_seed is not None else {}))

                if options.no_speech_threshold is not None:
                    skip = result.no_speech_prob > options.no_speech_threshold
                    if options.log_prob_threshold is not None and avg_logprob > options.log_prob_threshold:
                        skip = False            # confident text beats the no-speech probability
                    if skip:
                        seek += segment_size    # fast-forward to the next window
                        continue

                tokens = result.sequences_ids[0]
                current, seek, single_timestamp_ending = self._split_segments_by_timestamps(
                    tokenizer=tokenizer, tokens=tokens, time_offset=time_offset, segment_size=segment_size,
                    segment_duration=segment_duration, seek=seek)
                if extras.token_logprobs or extras.token_alternatives:
                    _slice_token_values(current, result.token_logprobs[0],
                                        result.token_alternatives[0] if extras.token_alternatives else None)

                if options.word_timestamps:
                    self.add_word_timestamps([current], tokenizer, encoder_output, segment_size,
                                             options.prepend_punctuations, options.append_punctuations,
                                             last_speech_timestamp=last_speech_timestamp)
                    seek, last_speech_timestamp, again = seek_after_words(
                        current, seek=seek, previous_seek=previous_seek, time_offset=time_offset,
                        segment_duration=segment_duration, window_end_time=window_end_time,
                        content_frames=content_frames, content_duration=content_duration, frames_per_second=fps,
                        single_timestamp_ending=single_timestamp_ending,
                        threshold=options.hallucination_silence_threshold, last_speech_timestamp=last_speech_timestamp)
                    if again:
                        continue

                for seg in current:
                    text = tokenizer.decode(seg["tokens"])
                    if seg["start"] == seg["end"] or not text.strip():
                        continue
                    all_tokens.extend(seg["tokens"])
                    idx += 1
                    values = dict(id=idx, seek=previous_seek, start=seg["start"], end=seg["end"], text=text,
                                  tokens=seg["tokens"], temperature=temperature, avg_logprob=avg_logprob,
                                  compression_ratio=compression_ratio, no_speech_prob=result.no_speech_prob,
                                  words=([Word(**w) for w in seg["words"]] if options.word_timestamps else None))
                    yield _make_segment(values, seg.get("token_logprobs"), seg.get("token_alternatives"))

                if not options.condition_on_previous_text or temperature > options.prompt_reset_on_temperature:
                    prompt_reset_since = len(all_tokens)
                if pbar is not None:
                    pbar.update((min(content_frames, seek) - previous_seek) * tpf)
        if pbar is not None:
            pbar.close()

    def generate_with_fallback(self, encoder_output: StorageView, prompt: List[int], tokenizer: Tokenizer,
                               options: TranscriptionOptions, sampling_seed: Optional[int] = None, seek: int = 0,
                               extras: DecodeExtras = DecodeExtras()):
        """Temperature ladder (transcribe.py:1402-1530): beam search at t = 0, `best_of` random samples at
        t > 0; a result is accepted unless it is too repetitive (compression ratio) or too improbable
        (average log-prob) — except when it looks like silence.  If every temperature fails, the most probable
        attempt (preferring those under the compression threshold) is returned with the last temperature.
        sampling_seed: the sampled attempt at rung t gets seed=attempt_seed(sampling_seed, seek, t), `seek` the window's
        first frame; None: no seed is passed, the backend draws one from its call counter.
        extras: the call's DecodeExtras, the same for every attempt; its sampling limits reach the sampled attempts
        (temperature > 0) only.
        -> (WhisperGenerationResult, avg_logprob, temperature, compression_ratio)"""
        max_initial_timestamp_index = int(round(options.max_initial_timestamp / self.time_precision))
        max_length = self._max_length_for(prompt, options.max_new_tokens)
        attempts, compact = [], []
        chosen = None
        for rung, temperature in enumerate(options.temperatures):
            if temperature > 0:
                mode = dict(beam_size=1, num_hypotheses=options.best_of, sampling_topk=0,
                            sampling_temperature=temperature)
                if sampling_seed is not None:
                    mode["seed"] = attempt_seed(sampling_seed, seek, rung)
            else:
                mode = dict(beam_size=options.beam_size, patience=options.patience)
            result = self.model.generate(
                encoder_output, [prompt], length_penalty=options.length_penalty,
                repetition_penalty=options.repetition_penalty, no_repeat_ngram_size=options.no_repeat_ngram_size,
                max_length=max_length, return_scores=True, return_no_speech_prob=True,
                suppress_blank=options.suppress_blank, suppress_tokens=options.suppress_tokens,
                max_initial_timestamp_index=max_initial_timestamp_index, **mode,
                **extras.generate_keywords(sampled=temperature > 0))[0]
            avg_logprob = _avg_logprob(result, options.length_penalty)
            compression_ratio = get_compression_ratio(tokenizer.decode(result.sequences_ids[0]).strip())
            attempt = (result, avg_logprob, temperature, compression_ratio)
            attempts.append(attempt)
            retry = False
            if options.compression_ratio_threshold is not None:
                if compression_ratio > options.compression_ratio_threshold:
                    retry = True
                else:
                    compact.append(attempt)
            low_prob = options.log_prob_threshold is not None and avg_logprob < options.log_prob_threshold
            if low_prob:
                retry = True
            if options.no_speech_threshold is not None and result.no_speech_prob > options.no_speech_threshold \
                    and low_prob:
                retry = False                   # silence: a colder decode will not help
            if not retry:
                chosen = attempt
                break
        if chosen is None:
            best = max(compact or attempts, key=lambda a: a[1])
            chosen = (best[0], best[1], temperature, best[3])   # last temperature drives the prompt reset
        return chosen

    def boost_list_for(self, boost_phrases, phrase_boost, tokenizer: Tokenizer):
        """The boost list of a transcribe() call (backend.Whisper.boost_list), or None without phrases.  Every phrase is
        encoded as " " + phrase.strip(), the form `hotwords` uses: ONE variant per phrase — the word as it stands after a
        space, in the caller's casing; a caller who wants the capitalised or the sentence-initial form boosted lists it as
        a phrase of its own.  All phrases get the strength phrase_boost (logit units; where phrases share a prefix the
        boost counts once: the list takes the maximum, not the sum).  phrase_boost has no default: no measurement on real
        speech stands behind any value, so phrases without a strength are a ValueError.  The list is built once per call
        and reused for every window, every attempt of the temperature ladder and every batch."""
        _check_boost_arguments(boost_phrases, phrase_boost)
        if boost_phrases is None:
            return None
        phrases = [tokenizer.encode(" " + p.strip()) for p in boost_phrases]
        if not phrases:
            return None
        return self.model.boost_list(phrases, [float(phrase_boost)] * len(phrases))

    def constraint_list_for(self, allowed_phrases, tokenizer: Tokenizer):
        """The constraint list of a transcribe() call (backend.Whisper.constraint_list), or None without phrases.  Every
        phrase is encoded as " " + phrase.strip(), as boost_phrases are: ONE variant per phrase, in the caller's casing.
        Every generate call of the transcription then returns exactly one phrase of the list (its timestamps apart), so
        EACH DECODED WINDOW IS ONE PHRASE: the keyword is meant for short clips and VAD-cut chunks — voice commands, form
        fields, re-recognition against an n-best list — not for running speech (a sequence of phrases is out of scope,
        as are grammars).  The decoding options must leave every phrase reachable, or the first generate call raises
        ValueError: with the default suppress_tokens=[-1] a phrase that contains a suppressed symbol is one (pass
        suppress_tokens=[] or drop the phrase), as are no_repeat_ngram_size > 0 and, with suppress_blank, a phrase whose
        first token is the blank.  The list is built once per call and reused for every window, every attempt of the
        temperature ladder, every batch and every recording."""
        _check_constraint_arguments(allowed_phrases)
        if allowed_phrases is None:
            return None
        phrases = [tokenizer.encode(" " + p.strip()) for p in allowed_phrases]
        if not phrases:
            return None
        return self.model.constraint_list(phrases)

    def make_tokenizer(self, task="transcribe", language="en") -> Tokenizer:
        return Tokenizer(self.hf_tokenizer, self.model.config, self.model.is_multilingual, task=task, language=language)

    # ---- backend wrappers -----------------------------------------------------------------
    def encode(self, features: np.ndarray) -> StorageView:
        to_cpu = self.model.device == "cuda" and len(self.model.device_index) > 1
        if features.ndim == 2:
            features = np.expand_dims(features, 0)
        return self.model.encode(StorageView.from_array(np.ascontiguousarray(features)), to_cpu=to_cpu)

    def get_prompt(self, tokenizer: Tokenizer, previous_tokens: List[int], without_timestamps: bool = False,
                   prefix: Optional[str] = None, hotwords: Optional[str] = None) -> List[int]:
        prompt = []
        half = self.max_length // 2
        if previous_tokens or (hotwords and not prefix):
            prompt.append(tokenizer.sot_prev)
            if hotwords and not prefix:
                hw = tokenizer.encode(" " + hotwords.strip())
                prompt.extend(hw[:half - 1] if len(hw) >= half else hw)
            if previous_tokens:
                prompt.extend(previous_tokens[-(half - 1):])
        prompt.extend(tokenizer.sot_sequence)
        if without_timestamps:
            prompt.append(tokenizer.no_timestamps)
        if prefix:
            pt = tokenizer.encode(" " + prefix.strip())
            if len(pt) >= half:
                pt = pt[:half - 1]
            if not without_timestamps:
                prompt.append(tokenizer.timestamp_begin)
            prompt.extend(pt)
        return prompt

    def _split_segments_by_timestamps(self, tokenizer: Tokenizer, tokens: List[int], time_offset: float,
                                      segment_size: int, segment_duration: float, seek: int):
        """consecutive-timestamp slicing of one chunk's tokens (transcribe.py:1024-1101)"""
        tb = tokenizer.timestamp_begin
        segs = []
        single_ts_end = len(tokens) >= 2 and tokens[-2] < tb <= tokens[-1]
        cuts = [i for i in range(1, len(tokens)) if tokens[i] >= tb and tokens[i - 1] >= tb]
        if cuts:
            if single_ts_end:
                cuts.append(len(tokens))
            last = 0
            for cur in cuts:
                piece = tokens[last:cur]
                segs.append(dict(seek=seek, start=time_offset + (piece[0] - tb) * self.time_precision,
                                 end=time_offset + (piece[-1] - tb) * self.time_precision, tokens=piece))
                last = cur
            if single_ts_end:
                seek += segment_size
            else:
                seek += (tokens[last - 1] - tb) * self.input_stride
        else:
            duration = segment_duration
            stamps = [t for t in tokens if t >= tb]
            if stamps and stamps[-1] != tb:
                duration = (stamps[-1] - tb) * self.time_precision
            segs.append(dict(seek=seek, start=time_offset, end=time_offset + duration, tokens=tokens))
            seek += segment_size
        return segs, seek, single_ts_end

    def find_alignment(self, tokenizer: Tokenizer, text_tokens: List[List[int]], encoder_output: StorageView,
                       num_frames, median_filter_width: int = 7) -> List[dict]:
        """per chunk: the words {word, tokens, start, end, probability} of its text tokens, timed by the
        backend's cross-attention DTW (transcribe.py:1698-1766).  `num_frames`: int or one int per chunk."""
        from .words import word_alignment
        if len(text_tokens) == 0:
            return []
        results = self.model.align(encoder_output, tokenizer.sot_sequence, text_tokens, num_frames,
                                   median_filter_width=median_filter_width)
        return [word_alignment(tokenizer, toks, res.alignments, res.text_token_probs, self.tokens_per_second)
                for res, toks in zip(results, text_tokens)]

    def add_word_timestamps(self, segments: List[List[dict]], tokenizer: Tokenizer, encoder_output: StorageView,
                            num_frames, prepend_punctuations: str, append_punctuations: str,
                            last_speech_timestamp: float) -> float:
        """`segments`: per chunk, the list of its sub-segment dicts (seek/start/end/tokens).  Aligns every
        chunk's text tokens in ONE backend call, merges punctuation into neighbouring words, clamps
        over-long words at sentence / pause / segment boundaries and stores `words` in every sub-segment
        (transcribe.py:1567-1696).  -> end time of the last word (carried into the next call)."""
        if len(segments) == 0:
            return None
        aligned = self.align_words(segments, tokenizer, encoder_output, num_frames, prepend_punctuations,
                                   append_punctuations)
        return self.apply_word_alignments(segments, aligned, last_speech_timestamp)

    def align_words(self, segments: List[List[dict]], tokenizer: Tokenizer, encoder_output: StorageView, num_frames,
                    prepend_punctuations: str, append_punctuations: str) -> List[dict]:
        """Chunk-local half of add_word_timestamps: one backend `align` call for all chunks, then per chunk the
        word list with sentence-boundary clamping and punctuation merged.  Needs the encoder output, i.e. runs
        on the rank that decoded the chunks; the result is plain data (picklable) for `apply_word_alignments`."""
        from .words import clamp_sentence_boundaries, merge_punctuations
        per_sub = [[[t for t in sub["tokens"] if t < tokenizer.eot] for sub in chunk] for chunk in segments]
        text_tokens = [[t for sub in subs for t in sub] for subs in per_sub]
        alignments = self.find_alignment(tokenizer, text_tokens, encoder_output, num_frames)
        out = []
        for alignment, subs in zip(alignments, per_sub):
            median, longest = clamp_sentence_boundaries(alignment)
            merge_punctuations(alignment, prepend_punctuations, append_punctuations)
            out.append(dict(words=alignment, median=median, longest=longest, tokens_per_subsegment=subs))
        return out

    def apply_word_alignments(self, segments: List[List[dict]], aligned: List[dict],
                              last_speech_timestamp: float) -> float:
        """Sequential half: distributes every chunk's words over its sub-segments; the pause heuristics chain
        through `last_speech_timestamp` from chunk to chunk, so this runs in chunk order on one process."""
        from .words import assign_words
        for chunk, a in zip(segments, aligned):
            last_speech_timestamp = assign_words(chunk, a["words"], a["tokens_per_subsegment"],
                                                 chunk[0]["seek"] / self.frames_per_second, a["median"], a["longest"],
                                                 last_speech_timestamp)
        return last_speech_timestamp

    def detect_language(self, audio: Optional[np.ndarray] = None, features: Optional[np.ndarray] = None,
                        vad_filter: bool = False, vad_parameters=None, language_detection_segments: int = 1,
                        language_detection_threshold: float = 0.5):
        assert audio is not None or features is not None, "Either `audio` or `features` must be provided."
        fe = self.feature_extractor
        if audio is not None:
            if vad_filter:   # keep only the speech before looking at the first segments (transcribe.py:1802-1806)
                from .vad import VadOptions, collect_chunks, get_speech_timestamps
                if isinstance(vad_parameters, dict):
                    vad_parameters = VadOptions(**vad_parameters)
                speech_chunks = get_speech_timestamps(audio, vad_parameters)
                audio = np.concatenate(collect_chunks(audio, speech_chunks)[0], axis=0)
            features = fe(audio[: language_detection_segments * fe.n_samples])
        features = features[..., : language_detection_segments * fe.nb_max_frames]
        return self._detect_language_segments(features, language_detection_threshold)

    def _detect_language_segments(self, features: np.ndarray, language_detection_threshold, first=None):
        """the loop over the 30 s segments of `features` until one is confident; first: the backend's detect_language
        result for segment 0 when the caller already has it (transcribe_many detects the first segments of many
        recordings in one batch)"""
        fe = self.feature_extractor
        seen = {}
        for i in range(0, features.shape[-1], fe.nb_max_frames):
            if i == 0 and first is not None:
                results = first
            else:
                enc = self.encode(pad_or_trim(features[..., i:i + fe.nb_max_frames]))
                results = self.model.detect_language(enc)[0]
            all_probs = [(tok[2:-2], p) for tok, p in results]
            language, prob = all_probs[0]
            if prob > language_detection_threshold:
                break
            seen.setdefault(language, []).append(prob)
        else:
            language = max(seen, key=lambda k: len(seen[k]))
            prob = max(seen[language])
        return language, prob, all_probs


@dataclass
class _Recording:
    """one recording on its way through the batched pipeline: cut into chunks by _split_recording, language (where it
    is detected) by the entry point's detection pass, the rest by _plan_decode"""
    audio: np.ndarray
    clip_timestamps: Optional[List[dict]]       # the caller's split, if any
    clips: List[dict]                           # the spans the chunks are cut from, in samples
    audio_chunks: List[np.ndarray]
    chunks_metadata: List[dict]
    duration_after_vad: float
    vad_options: object
    language: Optional[str] = None
    language_probability: float = 1
    all_language_probs: Optional[List[Tuple[str, float]]] = None
    tokenizer: Optional[Tokenizer] = None
    options: Optional[TranscriptionOptions] = None
    info: Optional[TranscriptionInfo] = None
    # transcribe_many: per chunk, in chunk order, its sub-segments and its word alignment
    decoded: List[List[dict]] = field(default_factory=list)
    aligned: List[dict] = field(default_factory=list)


class BatchedInferencePipeline:
    def __init__(self, model: WhisperModel):
        self.model = model
        self.last_speech_timestamp = 0.0

    # ---- one batch: encode + generate ---------------------------------------------------
    def generate_segment_batched(self, features, tokenizer: Tokenizer, options: TranscriptionOptions,
                                 audio_chunks: Optional[List[np.ndarray]] = None, extras: DecodeExtras = DecodeExtras()):
        """features: [B, n_mels, 3000] float32, or None when `audio_chunks` is given (fused resident
        PCM -> log-mel -> encoder path; the features never leave HBM).  extras.token_logprobs: every output dict also
        carries the chunk's per-token log-probs (`token_logprobs`) and that of its closing <eot> (`end_logprob`);
        extras.token_alternatives=N: those, and the N most likely (id, log-prob) pairs per token (`token_alternatives`) and
        at the closing <eot> (`end_alternatives`, None when the chunk was cut at the budget).  extras.boost /
        extras.constraint: the call's lists, passed to generate when there are any."""
        m = self.model
        batch_size = len(audio_chunks) if audio_chunks is not None else features.shape[0]
        prompt = m.get_prompt(tokenizer,
                              previous_tokens=(tokenizer.encode(options.initial_prompt)
                                               if isinstance(options.initial_prompt, str)
                                               else list(options.initial_prompt or [])),
                              without_timestamps=options.without_timestamps, hotwords=options.hotwords)
        max_length = m._max_length_for(prompt, options.max_new_tokens)
        encoder_output = m.model.encode_pcm(audio_chunks) if audio_chunks is not None else m.encode(features)
        prompts = [prompt.copy() for _ in range(batch_size)]
        if options.multilingual:
            names = language_token_strings(m.model.config)
            lang_tokens = [m.model.config.lang_begin + names.index(r[0][0]) for r in
                           m.model.detect_language(encoder_output)]
            idx = prompt.index(tokenizer.language)
            for i, t in enumerate(lang_tokens):
                prompts[i][idx] = t
        results = m.model.generate(
            encoder_output, prompts, beam_size=options.beam_size, patience=options.patience,
            length_penalty=options.length_penalty, max_length=max_length, suppress_blank=options.suppress_blank,
            suppress_tokens=options.suppress_tokens, return_scores=True, return_no_speech_prob=True,
            sampling_temperature=options.temperatures[0], repetition_penalty=options.repetition_penalty,
            no_repeat_ngram_size=options.no_repeat_ngram_size, **extras.generate_keywords())
        output = []
        for r in results:
            output.append(dict(avg_logprob=_avg_logprob(r, options.length_penalty), no_speech_prob=r.no_speech_prob,
                               tokens=r.sequences_ids[0]))
            if extras.token_logprobs or extras.token_alternatives:
                output[-1].update(token_logprobs=r.token_logprobs[0], end_logprob=r.end_logprobs[0])
            if extras.token_alternatives:
                output[-1].update(token_alternatives=r.token_alternatives[0], end_alternatives=r.end_alternatives[0])
        return encoder_output, output

    def forward(self, features, tokenizer, chunks_metadata, options, audio_chunks=None):
        encoder_output, outputs = self.generate_segment_batched(features, tokenizer, options, audio_chunks)
        segmented, sizes = self._split_outputs(outputs, tokenizer, chunks_metadata)
        if options.word_timestamps:
            self.last_speech_timestamp = self.model.add_word_timestamps(
                segmented, tokenizer, encoder_output, sizes, options.prepend_punctuations,
                options.append_punctuations, self.last_speech_timestamp)
        return segmented

    def _split_outputs(self, outputs, tokenizer, chunks_metadata):
        """per chunk: its sub-segment dicts (timestamp splitting) and its size in frames"""
        m = self.model
        segmented, sizes = [], []
        for meta, out in zip(chunks_metadata, outputs):
            duration = meta["duration"]
            size = int(ceil(duration) * m.frames_per_second)
            sizes.append(size)
            subs, _, _ = m._split_segments_by_timestamps(tokenizer=tokenizer, tokens=out["tokens"],
                                                         time_offset=meta["offset"], segment_size=size,
                                                         segment_duration=duration, seek=0)
            segmented.append([
                dict(text=tokenizer.decode(s["tokens"]), avg_logprob=out["avg_logprob"],
                     no_speech_prob=out["no_speech_prob"], tokens=s["tokens"], start=s["start"], end=s["end"],
                     compression_ratio=get_compression_ratio(tokenizer.decode(s["tokens"])),
                     seek=int(meta["offset"] * m.frames_per_second))
                for s in subs])
            if "token_logprobs" in out:
                _slice_token_values(segmented[-1], out["token_logprobs"], out.get("token_alternatives"))
        return segmented, sizes

    # ---- the public entry point ---------------------------------------------------------
    def transcribe(self, audio: Union[str, np.ndarray], language: Optional[str] = None, task: str = "transcribe",
                   log_progress: bool = False, beam_size: int = 5, best_of: int = 5, patience: float = 1,
                   length_penalty: float = 1, repetition_penalty: float = 1, no_repeat_ngram_size: int = 0,
                   temperature=(0.0, 0.2, 0.4, 0.6, 0.8, 1.0), compression_ratio_threshold: Optional[float] = 2.4,
                   log_prob_threshold: Optional[float] = -1.0, no_speech_threshold: Optional[float] = 0.6,
                   condition_on_previous_text: bool = True, prompt_reset_on_temperature: float = 0.5,
                   initial_prompt=None, prefix: Optional[str] = None, suppress_blank: bool = True,
                   suppress_tokens: Optional[List[int]] = [-1], without_timestamps: bool = True,
                   max_initial_timestamp: float = 1.0, word_timestamps: bool = False,
                   prepend_punctuations: str = "\"'“¿([{-", append_punctuations: str = "\"'.。,，!！?？:：”)]}、",
                   multilingual: bool = False, vad_filter: bool = True, vad_parameters=None,
                   max_new_tokens: Optional[int] = None, chunk_length: Optional[int] = None,
                   clip_timestamps: Optional[List[dict]] = None, hallucination_silence_threshold=None,
                   batch_size: int = 8, hotwords: Optional[str] = None,
                   language_detection_threshold: Optional[float] = 0.5, language_detection_segments: int = 1,
                   shard: bool = False, fused_features: bool = True, vad_speech_probs=None,
                   token_logprobs: bool = False, token_alternatives: int = 0,
                   boost_phrases: Optional[Sequence[str]] = None, phrase_boost: Optional[float] = None,
                   sampling_top_k: int = 0, sampling_top_p: float = 1.0,
                   allowed_phrases: Optional[Sequence[str]] = None):
        """Same contract as the reference (transcribe.py:254-578): returns (segment generator, info).
        token_logprobs=True (not in the reference): every segment is a ScoredSegment carrying the log-prob of each of
        its tokens; every other field is what the call without the keyword yields (not offered with shard=True).
        token_alternatives=N (not in the reference; 1 <= N <= backend.MAX_ALTERNATIVES): every segment is an
        AlternativesSegment, a ScoredSegment that also lists the N most likely (id, log-prob) pairs at the position of each
        of its tokens (not offered with shard=True either).
        shard=True: inside a torch.distributed job every rank calls this with the same arguments; the
        chunk list is block-partitioned over the ranks and rank 0's generator yields ALL segments in
        order (other ranks yield nothing).  fused_features=False reproduces the reference data flow
        (features materialised on the host, then encode()).
        boost_phrases, phrase_boost (not in the reference): see WhisperModel.boost_list_for — one list for every batch.
        sampling_top_k, sampling_top_p (not in the reference): WhisperModel.transcribe's limits on sampled attempts,
        validated here as there (ValueError).  They apply to the temperature > 0 rungs of the fallback ladder only, and the
        batched path decodes every chunk once, without sampling (as the reference's does): here they limit nothing.
        allowed_phrases (not in the reference): see WhisperModel.constraint_list_for — every chunk decodes to exactly one
        phrase of the list; one list for every batch.  Composes with boost_phrases."""
        args = dict(locals())               # the call's arguments by name
        from .vad import get_speech_timestamps
        m = self.model
        extras = _decode_extras(m, args)
        if (token_logprobs or token_alternatives) and shard:
            raise ValueError("token_logprobs / token_alternatives are not offered with shard=True: the gathered records "
                             "carry no per-token values")
        multilingual = m._effective_multilingual(multilingual)
        audio = np.asarray(m._load_audio(audio), dtype=np.float32)
        chunk_length = chunk_length or m.feature_extractor.chunk_length
        speech_spans = None
        if not clip_timestamps and vad_filter:
            vad_parameters = self._vad_options(vad_parameters, chunk_length)
            speech_spans = get_speech_timestamps(audio, vad_parameters, speech_probs=vad_speech_probs)
        rec = self._split_recording(audio, clip_timestamps, speech_spans, chunk_length, vad_parameters)
        if language is None and m.model.is_multilingual:
            rec.language, rec.language_probability, rec.all_language_probs = m.detect_language(
                features=self._language_features(rec.audio_chunks, language_detection_segments),
                language_detection_segments=language_detection_segments,
                language_detection_threshold=language_detection_threshold)
        self._plan_decode(rec, args, language, multilingual, {})
        gen = self._batched_segments_generator(rec.audio_chunks, rec.tokenizer, rec.chunks_metadata, batch_size,
                                               rec.options, log_progress, shard, fused_features, **extras.keyword())
        return self._on_recording_time(rec, gen), rec.info

    # ---- the steps of transcribe that transcribe_many runs per recording -----------------
    @staticmethod
    def _vad_options(vad_parameters, chunk_length):
        """the VAD options of the batched path: spans of at most one chunk"""
        from .vad import VadOptions
        if vad_parameters is None:
            return VadOptions(max_speech_duration_s=chunk_length, min_silence_duration_ms=160)
        if isinstance(vad_parameters, dict):
            return VadOptions(**{k: v for k, v in vad_parameters.items() if k != "max_speech_duration_s"},
                              max_speech_duration_s=chunk_length)
        return vad_parameters

    def _split_recording(self, audio, clip_timestamps, speech_spans, chunk_length, vad_options) -> "_Recording":
        """the record of one recording, cut into chunks.  clip_timestamps: the caller's split (wins); speech_spans: the
        VAD's spans of the recording (None: the VAD did not run); vad_options: what info.vad_options reports"""
        from .vad import collect_chunks
        m = self.model
        sr = m.feature_extractor.sampling_rate
        duration = audio.shape[0] / sr
        if not clip_timestamps:
            # no split provided: speech spans from the VAD (merged into <= chunk_length chunks), or the whole
            # audio when it is shorter than one chunk
            if speech_spans is not None:
                clips = speech_spans
            elif duration < chunk_length:
                clips = [{"start": 0, "end": audio.shape[0]}]
            else:
                raise RuntimeError("No clip timestamps found. Set 'vad_filter' to True or provide 'clip_timestamps'.")
            audio_chunks, chunks_metadata = collect_chunks(audio, clips, max_duration=chunk_length)
        else:
            clips = [{k: int(v * sr) for k, v in seg.items()} for seg in clip_timestamps]
            audio_chunks, chunks_metadata = [], []
            for i, clip in enumerate(clips):
                audio_chunks.append(audio[clip["start"]:clip["end"]])
                d = (clip["end"] - clip["start"]) / sr
                if d > 30:
                    m.logger.warning("Segment %d is longer than 30 seconds, only the first 30 seconds will be "
                                     "transcribed", i)
                chunks_metadata.append({"offset": clip["start"] / sr, "duration": d, "segments": [clip]})
        duration_after_vad = sum(c["end"] - c["start"] for c in clips) / sr
        # the reference formats the removed duration for its log line, which asserts it is not negative
        # (transcribe.py:458-461, utils.py:124): clips that add up to more than the recording are rejected
        assert duration - duration_after_vad >= 0, "non-negative timestamp expected"
        if not duration_after_vad:
            audio_chunks, chunks_metadata = [], []
        return _Recording(audio=audio, clip_timestamps=clip_timestamps, clips=clips, audio_chunks=audio_chunks,
                          chunks_metadata=chunks_metadata, duration_after_vad=duration_after_vad,
                          vad_options=vad_options)

    def _language_features(self, audio_chunks, language_detection_segments):
        """the features language detection looks at: the reference concatenates the (unpadded) features of ALL chunks;
        detect_language only looks at the first language_detection_segments * 3000 frames, so stop once those are covered"""
        m = self.model
        need = language_detection_segments * m.feature_extractor.nb_max_frames
        parts, have = [], 0
        for chunk in audio_chunks:
            if have >= need:
                break
            parts.append(m.feature_extractor(chunk)[..., :-1])
            have += parts[-1].shape[-1]
        # + one dummy frame so that empty audio still has a feature
        return np.concatenate(parts + [np.full((m.model.n_mels, 1), -1.5, dtype="float32")], axis=1)

    @staticmethod
    def _batched_options(args, tokenizer, clip_timestamps, multilingual) -> TranscriptionOptions:
        """args: transcribe()'s arguments by name.  The batched path decodes once, at the first temperature, every chunk
        on its own, and knows no hallucination skipping."""
        temperature, suppress_tokens = args["temperature"], args["suppress_tokens"]
        return _transcription_options(
            args, tokenizer, clip_timestamps=clip_timestamps, multilingual=multilingual,
            temperatures=(list(temperature[:1]) if isinstance(temperature, (list, tuple)) else [temperature]),
            suppress_tokens=(list(suppress_tokens) if suppress_tokens else suppress_tokens),
            hallucination_silence_threshold=None, condition_on_previous_text=False, prompt_reset_on_temperature=0.5,
            max_initial_timestamp=0.0)

    def _plan_decode(self, rec: "_Recording", args, language, multilingual, tokenizers) -> None:
        """what is left to decide before a recording's chunks can be decoded: its language (the argument, "en" for an
        English-only model, else what the detection pass has put into the record), tokenizer (one per language, kept in
        `tokenizers`), options and info.  args: transcribe()'s arguments by name."""
        m = self.model
        if language is not None:
            rec.language = m._effective_language(language)
        elif not m.model.is_multilingual:
            rec.language = "en"
        if rec.language not in tokenizers:
            tokenizers[rec.language] = m.make_tokenizer(task=args["task"], language=rec.language)
        rec.tokenizer = tokenizers[rec.language]
        rec.options = self._batched_options(args, rec.tokenizer, rec.clip_timestamps or rec.clips, multilingual)
        rec.info = TranscriptionInfo(
            language=rec.language, language_probability=rec.language_probability,
            duration=rec.audio.shape[0] / m.feature_extractor.sampling_rate, duration_after_vad=rec.duration_after_vad,
            transcription_options=rec.options, vad_options=rec.vad_options, all_language_probs=rec.all_language_probs)

    def _on_recording_time(self, rec: "_Recording", segments):
        """segments with their times on the recording's axis: chunks cut from speech spans carry times on the axis with
        the silence removed (the caller's clips are on the recording's axis already)"""
        if rec.clip_timestamps:
            return segments
        from .words import restore_speech_timestamps
        return restore_speech_timestamps(segments, rec.clips, self.model.feature_extractor.sampling_rate)

    def _batched_segments_generator(self, audio_chunks, tokenizer, chunks_metadata, batch_size, options,
                                    log_progress, shard=False, fused_features=True, extras=DecodeExtras()):
        from .sharding import gather_results, partition
        m = self.model
        rank, world, local_rank = 0, 1, 0
        if shard:
            import torch.distributed as dist
            rank, world = dist.get_rank(), dist.get_world_size()
            local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        n = len(audio_chunks)
        seg_idx = 0
        workers = m._workers()

        def batches(lo, hi):
            """(outs, local, aligned) per batch of the chunk range [lo, hi), in order, `workers` batches in flight"""
            spans = [(i, min(hi, i + batch_size)) for i in range(lo, hi, batch_size)]
            if workers >= 2 and len(spans) == 1 and hi - lo >= 4:
                # ONE batch and idle workers (a rank's share of a sharded recording: 1 h over 8 GPUs = 15 chunks): two
                # half batches on two workers — the second half's encoder pass runs under the first half's decode run and
                # the two runs decode side by side on the group's two lanes.  Results do not depend on the split (every
                # kernel works per chunk); measured 315 -> 290 ms for 15 chunks (profiles/r06_bench_c4_halves.json)
                mid = lo + (hi - lo + 1) // 2
                spans = [(lo, mid), (mid, hi)]
            return self._batches_in_flight([(audio_chunks[i0:i1], chunks_metadata[i0:i1], tokenizer, options)
                                            for i0, i1 in spans], shard, fused_features, **extras.keyword())

        def emit(results):
            nonlocal seg_idx
            for seg in self._segments(results, options, seg_idx + 1):
                seg_idx = seg.id
                yield seg

        if not shard:
            # single process: segments are yielded as soon as their batch is decoded
            for _, results, aligned in batches(0, n):
                if options.word_timestamps:
                    self.last_speech_timestamp = m.apply_word_alignments(results, aligned, self.last_speech_timestamp)
                yield from emit(results)
            self.last_speech_timestamp = 0.0
            return
        # sharded (a job of ONE rank takes this path too: same result, and the way a 1-GPU box executes the RCCL
        # gather): every rank decodes its contiguous block of the chunk list (no collective in the data path), then
        # ONE gather brings the fixed-size result records — and the chunk-local word alignments — to rank 0, in
        # rank order = the serial order
        bounds = partition(n, world)
        lo, hi = bounds[rank]
        max_len = m.max_length
        my_outs, my_aligned = [], []
        for outs, _, aligned in batches(lo, hi):
            my_outs.extend(outs)
            if options.word_timestamps:
                my_aligned.extend(aligned)
        counts = [b[1] - b[0] for b in bounds]
        ordered_aligned = None
        if options.word_timestamps:
            import torch.distributed as dist
            bucket = [None] * world if rank == 0 else None
            dist.gather_object(my_aligned, bucket, dst=0)
            if rank == 0:
                ordered_aligned = [a for r in range(world) for a in bucket[r]]
        got = gather_results(_OutRec.wrap(my_outs), max_len, rank, world, local_rank, counts=counts)
        if rank != 0:
            return
        ordered = [dict(tokens=ids, avg_logprob=avg_lp, no_speech_prob=nsp) for (ids, avg_lp, nsp) in got]
        results, _ = self._split_outputs(ordered, tokenizer, chunks_metadata)
        if options.word_timestamps:
            self.last_speech_timestamp = m.apply_word_alignments(results, ordered_aligned, self.last_speech_timestamp)
        yield from emit(results)
        self.last_speech_timestamp = 0.0

    def _decode_batch(self, chunks, chunks_metadata, tokenizer, options, shard=False, fused_features=True,
                      extras=DecodeExtras()):
        """one batch: encode + generate, then the chunk-local post-processing -> (outs, sub-segments, word alignments)"""
        m = self.model
        feats = None if fused_features else m.model.log_mel(chunks)
        enc, outs = self.generate_segment_batched(feats, tokenizer, options,
                                                  audio_chunks=chunks if fused_features else None, **extras.keyword())
        local = aligned = None
        if not shard or options.word_timestamps:
            local, sizes = self._split_outputs(outs, tokenizer, chunks_metadata)
            if options.word_timestamps:
                # the chunk-local half of the word timing runs where the encoder output lives
                aligned = m.align_words(local, tokenizer, enc, sizes, options.prepend_punctuations,
                                        options.append_punctuations)
        return outs, local, aligned

    def _batches_in_flight(self, jobs, shard=False, fused_features=True, extras=DecodeExtras()):
        """(outs, local, aligned) per job = (chunks, chunks_metadata, tokenizer, options), in order.
        The batches are independent (`condition_on_previous_text=False`): with worker replicas
        (WhisperModel(num_workers=W) -> backend inter_threads) W batches are kept in flight on the GPU — their
        encoders run side by side and their generate() calls share decode runs (backend decode groups).  Only
        the word-timestamp pause heuristics chain through last_speech_timestamp; those run in order, in the caller."""
        workers = self.model._workers()
        if workers <= 1 or len(jobs) <= 1:
            for job in jobs:
                yield self._decode_batch(*job, shard, fused_features, **extras.keyword())
            return
        from collections import deque
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(max_workers=workers) as pool:
            pending = deque()
            for job in jobs:
                pending.append(pool.submit(self._decode_batch, *job, shard, fused_features, **extras.keyword()))
                if len(pending) >= workers:
                    yield pending.popleft().result()
            while pending:
                yield pending.popleft().result()

    @staticmethod
    def _segments(results, options, first_id):
        """the Segment objects of decoded chunks (`results`: per chunk its sub-segment dicts), ids from first_id"""
        idx = first_id
        for result in results:
            for seg in result:
                values = dict(seek=seg["seek"], id=idx, text=seg["text"], start=round(seg["start"], 3),
                              end=round(seg["end"], 3), tokens=seg["tokens"], avg_logprob=seg["avg_logprob"],
                              words=(None if not options.word_timestamps else [Word(**w) for w in seg["words"]]),
                              no_speech_prob=seg["no_speech_prob"], compression_ratio=seg["compression_ratio"],
                              temperature=options.temperatures[0])
                # (sub-segments carry token_logprobs exactly when the call asked for them: _split_outputs)
                yield _make_segment(values, seg.get("token_logprobs"), seg.get("token_alternatives"))
                idx += 1

    # ---- many recordings in one call ------------------------------------------------------------
    def transcribe_many(self, audios: Sequence[Union[str, np.ndarray]], *, language=None, clip_timestamps=None,
                        vad_speech_probs=None, vad_model=None, shard: bool = False,
                        **kwargs) -> List[Tuple[List[Segment], TranscriptionInfo]]:
        """Transcribes several recordings in ONE call: result[i] = (list of segments, info) is what
        `BatchedInferencePipeline(model).transcribe(audios[i], ...)` on a fresh pipeline yields, field for field (the
        engine's result for a chunk does not depend on what shares its batch), but the work is shared: one VAD pass
        over all recordings (`vad_model.forward_many`), first-segment language detection in batches, and the chunks of
        ALL recordings pooled into batches of `batch_size` — cut across recording boundaries, `num_workers` batches in
        flight — so a thousand 20 s clips run the encoder and the decoder as full batches, not a thousand batches of one.

        language, clip_timestamps, vad_speech_probs: one value for all recordings, or a sequence with one entry per
        recording.  vad_model: a SileroVADModel or a callable (default: get_vad_model()).  Every other keyword is
        transcribe()'s, with its default.  A batch holds chunks of one language (the prompt is per language).  Returns
        when every recording is done; shard=True is not offered here (ValueError)."""
        import inspect
        from .vad import get_speech_timestamps_many
        if shard:
            raise ValueError("transcribe_many does not shard: call it per rank on that rank's recordings")
        a = inspect.signature(self.transcribe).bind(None, **kwargs)     # transcribe's keywords and defaults
        a.apply_defaults()
        a = a.arguments
        m = self.model
        n = len(audios)
        extras = _decode_extras(m, a)     # (ONE list of either kind for the batches of every recording and language)
        if n == 0:
            return []
        multilingual = m._effective_multilingual(a["multilingual"])
        languages = _per_recording(language, n, "language", lambda v: v is None or isinstance(v, str))
        clip_lists = _per_recording(clip_timestamps, n, "clip_timestamps",
                                    lambda v: v is None or all(isinstance(c, dict) for c in v))
        probs = _per_recording(vad_speech_probs, n, "vad_speech_probs",
                               lambda v: v is None or isinstance(v, np.ndarray)
                               or all(np.ndim(p) == 0 and p is not None for p in v))
        audios = [np.asarray(m._load_audio(audio), dtype=np.float32) for audio in audios]
        chunk_length = a["chunk_length"] or m.feature_extractor.chunk_length

        # ---- VAD: one pass over every recording that needs it ----
        spans, vad_options = [None] * n, [a["vad_parameters"]] * n
        need_vad = [r for r in range(n) if not clip_lists[r] and a["vad_filter"]]
        if need_vad:
            opts = self._vad_options(a["vad_parameters"], chunk_length)
            found = get_speech_timestamps_many([audios[r] for r in need_vad], opts, vad_model=vad_model,
                                               speech_probs=[probs[r] for r in need_vad])
            for r, found_spans in zip(need_vad, found):
                spans[r], vad_options[r] = found_spans, opts

        # ---- plan: every recording cut into chunks ----
        recs = [self._split_recording(audio, clips, speech_spans, chunk_length, options)
                for audio, clips, speech_spans, options in zip(audios, clip_lists, spans, vad_options)]

        # ---- detect: the first detection segment of all undecided recordings in batches; then language, tokenizer
        #      (one per language), options and info of every recording ----
        if m.model.is_multilingual:
            frames = m.feature_extractor.nb_max_frames
            undecided = [(rec, self._language_features(rec.audio_chunks, a["language_detection_segments"])
                          [..., :a["language_detection_segments"] * frames])
                         for rec, given in zip(recs, languages) if given is None]
            for i in range(0, len(undecided), a["batch_size"]):
                part = undecided[i:i + a["batch_size"]]
                enc = m.encode(np.stack([pad_or_trim(feats[..., :frames]) for _, feats in part]))
                for (rec, feats), first in zip(part, m.model.detect_language(enc)):
                    # (a recording whose first segment stays under the threshold goes on alone with its further segments)
                    rec.language, rec.language_probability, rec.all_language_probs = m._detect_language_segments(
                        feats, a["language_detection_threshold"], first=first)
        tokenizers = {}
        for rec, given in zip(recs, languages):
            self._plan_decode(rec, a, given, multilingual, tokenizers)

        # ---- pool: the chunks of all recordings in recording order, per language; a batch every batch_size chunks ----
        jobs, owners = [], []                                  # owners[j]: the recording of every chunk of job j
        for tokenizer in tokenizers.values():
            same_language = [rec for rec in recs if rec.tokenizer is tokenizer]
            pool = [(rec, chunk, meta) for rec in same_language
                    for chunk, meta in zip(rec.audio_chunks, rec.chunks_metadata)]
            # (what a batch's decode reads of the options is the same for every recording of a language: they differ in
            #  clip_timestamps alone)
            options = same_language[0].options
            for i in range(0, len(pool), a["batch_size"]):
                part = pool[i:i + a["batch_size"]]
                jobs.append(([chunk for _, chunk, _ in part], [meta for _, _, meta in part], tokenizer, options))
                owners.append([rec for rec, _, _ in part])

        # ---- route: every chunk's sub-segments and word alignment back to its recording, in chunk order ----
        for owner, (_, local, aligned) in zip(owners, self._batches_in_flight(jobs, False, a["fused_features"],
                                                                              **extras.keyword())):
            for j, rec in enumerate(owner):
                rec.decoded.append(local[j])
                if aligned is not None:
                    rec.aligned.append(aligned[j])
        out = []
        for rec in recs:
            if a["word_timestamps"]:
                m.apply_word_alignments(rec.decoded, rec.aligned, 0.0)   # the pause heuristics chain within a recording
            segments = self._on_recording_time(rec, self._segments(rec.decoded, rec.options, 1))
            out.append((list(segments), rec.info))
        return out


class _OutRec:
    """adapts the pipeline's per-chunk dicts to the record layout of sharding.gather_results
    (ids, one float score slot = avg_logprob, no_speech_prob)"""

    def __init__(self, d):
        self.sequences_ids = [d["tokens"]]
        self.scores = [d["avg_logprob"]]
        self.no_speech_prob = d["no_speech_prob"]

    @staticmethod
    def wrap(outs):
        return [_OutRec(o) for o in outs]
