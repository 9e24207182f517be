"""Request / configuration types of the engine boundary (B4 of SURVEY.md section 8b).

Pure data classes; names, fields, defaults and enum values are those of the reference's
chirrup/core_structure.py (Task :92-169, ModelLoadConfig :182-232, RequestStatus :61-82,
FinishReason :40-55, defaults :13-36) because the worker protocol and the OpenAI surface are
written against them.  No arithmetic lives here.
"""
import enum
import math
import numbers
import operator
import queue
import uuid
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional

import torch

FINISH_REASON_STRINGS = ("stop", "length", "abort")
DEFAULT_STOP_TOKENS = [0, 261, 24281]
DEFAULT_SAMPLING_CONFIG: Dict[str, Any] = {
    "temperature": 1.0,
    "top_p": 0.3,
    "top_k": 0,
    "presence_penalty": 0.5,
    "frequency_penalty": 0.5,
    "penalty_decay": 0.996,
    "max_tokens": 8192,
}
LOGIT_BIAS_MAX = 1024          # entries of one request's logit_bias (the worker's per-slot list capacity)
EMBED_POOLINGS = ("mean", "last")   # Task.embed
BEAM_WIDTH_MAX = 8             # Task.beam_width
BEAM_K_MAX = 20                # candidates per beam and step, beam_width + len(stop_tokens): the top-K of the log-prob kernel (ops.TOP_LOGPROBS_MAX)
GUIDE_STACK_DEPTH_MAX = 32     # pushes a grammar guide's per-slot stack holds (guided.compile_grammar: max_depth)
GUIDE_CALL_SITES_MAX = 255     # call sites of one grammar guide: a stack level is one byte, 0 the bottom marker
GUIDE_MAX_STATES = 4096        # states of one guide's byte DFA (chirrup_amd/guided.py); a state is one row of the worker's guide pool


class FinishReason(enum.IntEnum):
    STOP = 0
    LENGTH = 1
    ABORT = 2

    def __str__(self):
        return FINISH_REASON_STRINGS[self.value]


class RequestStatus(enum.IntEnum):
    WAITING = enum.auto()
    RUNNING = enum.auto()
    FINISHED = enum.auto()              # everything above this value is a terminal state
    FINISHED_STOPPED = enum.auto()
    FINISHED_LENGTH_CAPPED = enum.auto()
    FINISHED_ABORTED = enum.auto()

    def __str__(self):
        return self.name

    @staticmethod
    def is_finished(status: "RequestStatus") -> bool:
        return status > RequestStatus.FINISHED

    @staticmethod
    def get_finished_reason(status: "RequestStatus") -> Optional[FinishReason]:
        return {RequestStatus.FINISHED_STOPPED: FinishReason.STOP,
                RequestStatus.FINISHED_LENGTH_CAPPED: FinishReason.LENGTH,
                RequestStatus.FINISHED_ABORTED: FinishReason.ABORT}.get(status)


@dataclass
class Task:
    """One generation request.  ``output_queue`` receives ("token_generated", (id, text[, logits])) -- (id, text, logits or None,
    logprobs) when ``logprobs`` is set --
    ("cache_prefill", {"state", "prefilled_tokens"}), ("beams", {...}) (beam search) and ("task_completed", task) tuples;
    ``task_event_queue`` carries ("abort", payload) from the front end."""

    output_queue: Any
    task_event_queue: queue.Queue
    prompt_str: str
    prefill_tokens: List[int]
    state: Optional[List[torch.Tensor]]
    task_id: Optional[str] = None
    priority: int = 0

    temperature: float = DEFAULT_SAMPLING_CONFIG["temperature"]
    top_p: float = DEFAULT_SAMPLING_CONFIG["top_p"]
    top_k: int = DEFAULT_SAMPLING_CONFIG["top_k"]
    presence_penalty: float = DEFAULT_SAMPLING_CONFIG["presence_penalty"]
    frequency_penalty: float = DEFAULT_SAMPLING_CONFIG["frequency_penalty"]
    penalty_decay: float = DEFAULT_SAMPLING_CONFIG["penalty_decay"]
    max_tokens: Optional[int] = DEFAULT_SAMPLING_CONFIG["max_tokens"]

    stop_tokens: List[int] = field(default_factory=lambda: DEFAULT_STOP_TOKENS)
    forbidden_tokens: List[int] = field(default_factory=list)

    cache_prefill: bool = False
    cache_prefill_padding: int = 0
    return_logits: bool = False
    # log-probabilities of the raw model output (before forbidden tokens, penalties, temperature and top-p / top-k) of each
    # generated token and of the top_logprobs (0..20) most likely ids: a fourth element {"logprob", "top_logprobs"} of the
    # ("token_generated", ...) payload; a forbidden token can therefore appear among the top_logprobs
    logprobs: bool = False
    top_logprobs: int = 0
    # sampled rows draw from Philox4x32-10 keyed by this seed (an int64 is read as its two's complement uint64), one counter per
    # sampled token: the ids then depend on (seed, draw index) and the logits only, not on the slot or the other requests
    seed: Optional[int] = None
    # {token id: bias}: added to the raw logits (binary32, one rounding to binary16, clamped to +-65504) after the forbidden
    # tokens and before the penalties; it moves greedy rows too, and logprobs still measure the raw output
    logit_bias: Dict[int, float] = field(default_factory=dict)
    # prompt logprobs (None: off; k in 0..20): position i >= 1 of prefill_tokens gets the log-softmax of the raw model output after
    # tokens < i taken at token i, plus the k most likely ids -- ("prompt_logprobs", {"start", "token_ids", "logprobs",
    # "top_logprobs"}) messages in position order before the first token; position 0 is None.  With max_tokens=0 the request only
    # scores: it ends (length) once the last position is known, without feeding the last prompt token or sampling anything
    prompt_logprobs: Optional[int] = None
    # parallel choices (n) of one prompt: the group's first task (choice 0) carries the others (choices 1..n-1, each with its own
    # queues, tables and finish) in `siblings`; the worker admits the group into n slots at once, prefills the prompt once and copies
    # the state into the siblings' slots before the last prompt token (DESIGN.md "Parallel choices (n)").  A seeded choice j draws
    # from Philox stream j, so choice 0 reproduces the single request with the same seed
    choice_index: int = 0
    siblings: List["Task"] = field(default_factory=list)
    # guided decoding: a guided.ByteDFA the generated text must match in full.  Each decode step masks the tokens whose bytes would
    # leave the automaton; a stop token is allowed in accepting states only, so "stop" means the text matches (max_tokens may still
    # cut it short).  Needs stop tokens and max_tokens > 0; logprobs still measure the raw output (DESIGN.md "Guided decoding")
    guide: Any = None
    # text embedding ("mean" | "last"; None: an ordinary request): the request only prefills -- every prompt token is fed, the last
    # one too -- and answers ("embedding", {"embedding", "pooled_tokens", "prompt_tokens"}): the binary16 ln_out rows (what the head
    # would multiply) of the prompt positions >= embed_skip, averaged or the last one, L2-normalised when embed_normalize.  Nothing
    # is sampled, so the sampling fields are ignored (DESIGN.md "Embeddings")
    embed: Optional[str] = None
    embed_skip: int = 0
    embed_normalize: bool = True
    # beam search (0: off; a width W in 2..BEAM_WIDTH_MAX): the request holds W slots and answers ONE ("beams", {"hypotheses",
    # "prompt_tokens"}) message (prompt_tokens: the tokens fed -- behind a prefix-cache hit, the uncached remainder) with its
    # beam_n_best (1..W) best hypotheses, ranked by cumulative_logprob / max(T, 1)**length_penalty (T text tokens), each {"token_ids", "text", "cumulative_logprob", "score", "finish_reason"}; nothing streams.  It needs
    # 1 <= len(stop_tokens) <= BEAM_K_MAX - W and max_tokens > 0.  The search reads the raw model output: temperature, top_p, top_k,
    # seed and the penalty fields are accepted and ignored (DESIGN.md "Beam search")
    beam_width: int = 0
    length_penalty: float = 1.0
    beam_n_best: int = 1

    event_list: List = field(init=False, default_factory=list)
    request_status: RequestStatus = field(init=False, default=RequestStatus.WAITING)
    error: Optional[str] = field(init=False, default=None)      # why the worker refused the request (it then ends aborted)
    generated_tokens: List[int] = field(init=False, default_factory=list)
    decoded_texts: List[str] = field(init=False, default_factory=list)

    def __post_init__(self):
        if self.task_id is None:
            self.task_id = str(uuid.uuid4())
        if not 0 <= self.top_logprobs <= 20 or (self.top_logprobs > 0 and not self.logprobs):
            raise ValueError("top_logprobs must be in 0..20, and a value > 0 requires logprobs")
        if self.seed is not None:
            self.seed = _integer(self.seed, "seed")
            if not -(1 << 63) <= self.seed < (1 << 64):
                raise ValueError("seed must be an integer in [-2^63, 2^64)")
        if self.prompt_logprobs is not None:
            self.prompt_logprobs = _integer(self.prompt_logprobs, "prompt_logprobs")
            if not 0 <= self.prompt_logprobs <= 20:
                raise ValueError("prompt_logprobs must be None or in 0..20")
        bias = dict(self.logit_bias or {})
        if len(bias) > LOGIT_BIAS_MAX:
            raise ValueError(f"logit_bias holds {len(bias)} entries, at most {LOGIT_BIAS_MAX} are allowed")
        checked = {}
        for t, v in bias.items():
            t = _integer(t, "logit_bias token id")
            if t < 0 or t in checked:
                raise ValueError(f"logit_bias: token id {t} is negative or repeated")
            if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v):
                raise ValueError(f"logit_bias: the bias of token {t} is not a finite number")
            checked[t] = float(v)
        self.logit_bias = checked
        if self.guide is not None:
            if not all(hasattr(self.guide, a) for a in ("next", "accept", "key")):
                raise ValueError("guide must be a guided.ByteDFA (compile_regex, compile_choice)")
            if not self.stop_tokens:
                raise ValueError("a guided request needs stop tokens: the end of a constrained text is a stop token")
            if self.max_tokens == 0 or self.prompt_logprobs is not None:
                raise ValueError("a guide applies to generated tokens only: not with max_tokens=0 or prompt_logprobs")
        self.check_group()
        self.check_beam()
        if self.embed is not None:
            if self.embed not in EMBED_POOLINGS:
                raise ValueError(f"embed: unknown pooling {self.embed!r}, expected one of {', '.join(EMBED_POOLINGS)}")
            self.embed_skip = _integer(self.embed_skip, "embed_skip")
            for name, on in (("logprobs", self.logprobs), ("prompt_logprobs", self.prompt_logprobs is not None),
                             ("return_logits", self.return_logits), ("guide", self.guide is not None),
                             ("siblings", bool(self.siblings)), ("choice_index > 0", self.choice_index > 0),
                             ("cache_prefill", self.cache_prefill), ("state", self.state is not None)):
                if on:
                    raise ValueError(f"embed cannot be combined with {name}")
            if self.embed_skip < 0 or len(self.prefill_tokens) - self.embed_skip < 1:
                raise ValueError(f"embed: no prompt position to pool ({len(self.prefill_tokens)} tokens, embed_skip {self.embed_skip})")

    def check_group(self) -> None:
        """Validates choice_index and siblings (at construction, and by whoever assembles a group afterwards)."""
        self.choice_index = _integer(self.choice_index, "choice_index")
        self.siblings = list(self.siblings or [])
        if self.choice_index < 0 or (self.siblings and self.choice_index != 0):
            raise ValueError("choice_index must be >= 0, and 0 for the task that carries the siblings")
        for j, sib in enumerate(self.siblings, start=1):
            if not isinstance(sib, Task) or sib.siblings or sib.choice_index != j:
                raise ValueError(f"sibling {j} must be a Task with choice_index {j} and no siblings of its own")
        if any(getattr(t, "embed", None) is not None for t in [self] + self.siblings) and (self.siblings or self.choice_index > 0):
            raise ValueError("embed cannot be combined with siblings / choice_index > 0")
        if self.siblings:
            if any(t.prompt_logprobs is not None for t in [self] + self.siblings):
                raise ValueError("parallel choices (n > 1) cannot be combined with prompt_logprobs")
            if any(t.max_tokens == 0 for t in [self] + self.siblings):
                raise ValueError("parallel choices (n > 1) need max_tokens > 0")

    def check_beam(self) -> None:
        """Validates the beam-search fields and what a beam request cannot be combined with (at construction)."""
        self.beam_width = _integer(self.beam_width, "beam_width")
        self.beam_n_best = _integer(self.beam_n_best, "beam_n_best")
        lam = self.length_penalty
        if isinstance(lam, bool) or not isinstance(lam, numbers.Real) or not math.isfinite(lam):
            raise ValueError(f"length_penalty must be a finite number, got {lam!r}")
        self.length_penalty = float(lam)
        if self.beam_width == 0:
            if self.beam_n_best != 1:
                raise ValueError("beam_n_best needs beam_width")
            return
        W = self.beam_width
        if not 2 <= W <= BEAM_WIDTH_MAX:
            raise ValueError(f"beam_width must be 0 (off) or in 2..{BEAM_WIDTH_MAX}, got {W}")
        if not 1 <= self.beam_n_best <= W:
            raise ValueError(f"beam_n_best must be in 1..beam_width ({W}), got {self.beam_n_best}")
        stops = set(self.stop_tokens or [])
        if not 1 <= len(stops) <= BEAM_K_MAX - W:
            raise ValueError(f"beam search needs 1..{BEAM_K_MAX - W} distinct stop tokens at beam_width {W}, got {len(stops)}")
        if self.max_tokens is None or self.max_tokens == 0:
            raise ValueError("beam search needs max_tokens > 0")
        for name, on in (("logprobs", self.logprobs), ("return_logits", self.return_logits),
                         ("prompt_logprobs", self.prompt_logprobs is not None), ("guide", self.guide is not None),
                         ("logit_bias", bool(self.logit_bias)), ("forbidden_tokens", bool(self.forbidden_tokens)),
                         ("embed", self.embed is not None), ("siblings", bool(self.siblings)),
                         ("choice_index > 0", self.choice_index > 0)):
            if on:
                raise ValueError(f"beam search cannot be combined with {name}")

    def is_finished(self) -> bool:
        return RequestStatus.is_finished(self.request_status)


def _integer(x, what: str) -> int:
    if isinstance(x, bool):
        raise ValueError(f"{what} must be an integer, got {x!r}")
    try:
        return operator.index(x)
    except TypeError:
        raise ValueError(f"{what} must be an integer, got {x!r}") from None


@dataclass
class ModelLoadConfig:
    model_path: str
    vocab_path: str
    vocab_size: int
    head_size: int
    dtype: object = torch.float16            # torch.int8 selects the mm8 (w8a16) channel-mix path, "mxfp4" the MXFP4 (w4a16) one
    att_dtype: torch.dtype = torch.float16   # (not in the reference) torch.int8: receptance / key / value / output and the head as mm8 too

    n_head: Optional[int] = field(default=None, init=False)
    n_embd: Optional[int] = field(default=None, init=False)
    n_layer: Optional[int] = field(default=None, init=False)

    @property
    def param_byte(self) -> int:
        return {torch.float16: 2, torch.float32: 4, torch.bfloat16: 2, torch.int8: 1}.get(self.dtype, 2)

    def load_params(self, n_head: int, n_embd: int, n_layer: int) -> None:
        self.n_head, self.n_embd, self.n_layer = n_head, n_embd, n_layer

    def get_state_size_mb(self) -> float:
        """Per-request state in MB, with the reference's formula (core_structure.py:210-232: it counts
        vocab_size elements for state[2])."""
        if self.n_layer is None or self.n_embd is None:
            raise ValueError("n_layer and n_embd must be set through load_params first")
        n = self.n_layer * 2 * self.n_embd + self.n_layer * (self.n_embd // self.head_size) * self.head_size ** 2
        return (n + self.vocab_size) * self.param_byte / (1024 * 1024)
