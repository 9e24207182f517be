"""OpenAI-compatible surface over AsyncEngineCore (SURVEY.md section 8 f/4; reference: chirrup/web_service/app.py:128-330,
api_model.py:8-112, chirrup/utils/prompt_formatters.py, streaming_string_parser.py).  Thin by design: `GET /health`,
`GET /v1/models`, `POST /v1/chat/completions` (streamed as server-sent events, or one JSON body) -- the reference's request
fields, chat template (`User:/Assistant:` paragraphs, model suffixes `:thinking` / `:no-thinking`), `[0]` + encode,
prefix-state cache protocol (`check_and_wait_prefill` -> `completion(state=...)` -> `cache()` + `awake_hang_up_prefills` on the
("cache_prefill", ...) event; in process mode the states are arena row addresses and never leave HBM) and 10-s keep-alive comments.
`POST /v1/completions` is OpenAI's legacy text route (not in the reference): raw prompts, and with `echo` + `logprobs` the scores of
the prompt's own tokens (prompt logprobs, `max_tokens=0` to score only) -- what evaluation harnesses call.
`POST /v1/embeddings` is OpenAI's embeddings route (not in the reference either): one vector per input, the pooled hidden state in
front of the head (DESIGN.md "Embeddings").
Not here: the settings CLI and the batch translate / rollout routes (out of scope).

    app = create_app(engine, state_cache_size=50)       # engine: an initialised AsyncEngineCore
"""
import asyncio
import base64
import json
import math
import re
import time
import uuid
from typing import Any, Dict, List, Literal, Optional, Tuple, Union

from fastapi import FastAPI, HTTPException
from fastapi.responses import StreamingResponse
from pydantic import BaseModel, Field, model_validator

from .core_structure import BEAM_K_MAX, DEFAULT_SAMPLING_CONFIG, DEFAULT_STOP_TOKENS, EMBED_POOLINGS, LOGIT_BIAS_MAX, RequestStatus
from .guided import GuideError
from .state_cache import SimpleStateCache

KEEP_ALIVE_S = 10.0
EMBEDDING_INPUTS_MAX = 2048      # inputs of one /v1/embeddings request (OpenAI's limit)
_SSE_HEADERS = {"Cache-Control": "no-cache", "Connection": "keep-alive", "X-Accel-Buffering": "no"}


class ChatMessage(BaseModel):
    role: str
    content: str
    reasoning_content: Optional[str] = None


def _check_logit_bias(logit_bias: Optional[Dict[str, float]]) -> None:
    seen = set()
    for key, value in (logit_bias or {}).items():
        if not re.fullmatch(r"[0-9]+", key):
            raise ValueError(f"logit_bias: key {key!r} is not a token id")
        if int(key) in seen:
            raise ValueError(f"logit_bias: token id {int(key)} appears twice")
        seen.add(int(key))
        if not -100.0 <= value <= 100.0:
            raise ValueError(f"logit_bias: the bias of token {key} is outside [-100, 100]")
    if len(seen) > LOGIT_BIAS_MAX:
        raise ValueError(f"logit_bias: at most {LOGIT_BIAS_MAX} entries")


def guided_arguments(engine, request, thinking: bool = False) -> Dict[str, Any]:
    """The guided_* keywords of engine.completion() for a request's guided_regex / guided_choice / guided_grammar / response_format, checked and
    compiled now: every refusal is a 400 with the reason (more than one of them, json_object, a pattern or schema outside the
    supported subset, a guide on a model variant that opens with a reasoning block)."""
    kw: Dict[str, Any] = {}
    if request.guided_regex is not None:
        kw["guided_regex"] = request.guided_regex
    if request.guided_choice is not None:
        kw["guided_choice"] = request.guided_choice
    rf = request.response_format
    if rf is not None and rf.get("type") != "text":
        if rf.get("type") == "json_object":
            raise HTTPException(status_code=400, detail="response_format json_object is not supported: arbitrary JSON nests without bound "
                                "and is not a regular language; give a schema with response_format json_schema")
        schema = (rf.get("json_schema") or {}).get("schema") if isinstance(rf.get("json_schema"), dict) else None
        if rf.get("type") != "json_schema" or not isinstance(schema, dict):
            raise HTTPException(status_code=400, detail="response_format: expected {\"type\": \"text\"} or {\"type\": \"json_schema\", "
                                "\"json_schema\": {\"schema\": {...}}}")
        kw["guided_json"] = schema
    if request.guided_grammar is not None:
        kw["guided_grammar"] = request.guided_grammar
        if len(kw) > 1:
            raise HTTPException(status_code=400, detail="at most one of guided_regex, guided_choice, guided_grammar and response_format "
                                f"json_schema may be given, got {len(kw)}")
    if len(kw) > 1:
        raise HTTPException(status_code=400, detail=f"at most one of guided_regex, guided_choice and response_format json_schema may be given, got {len(kw)}")
    if kw and thinking:
        raise HTTPException(status_code=400, detail="guided decoding cannot follow a reasoning block: use a model without the :thinking suffix")
    try:
        engine.compile_guide(**kw)
    except GuideError as e:
        raise HTTPException(status_code=400, detail=f"guided decoding: {e}")
    return kw


BEAM_WIDTH_DEFAULT = 4


def beam_arguments(engine, request, logprobs: bool, thinking: bool = False, n: int = 1) -> Dict[str, Any]:
    """The engine keywords of a request's beam-search fields ({} without use_beam_search); every combination beam search excludes
    answers 400 with the conflict named, before anything is queued."""
    if not request.use_beam_search:
        if request.beam_width is not None:
            raise HTTPException(status_code=400, detail="beam_width needs use_beam_search: true")
        return {}
    W = request.beam_width if request.beam_width is not None else BEAM_WIDTH_DEFAULT
    conflicts = [name for name, on in (("stream", request.stream), ("logprobs", logprobs), ("logit_bias", bool(request.logit_bias)),
                                       ("guided_regex", request.guided_regex is not None),
                                       ("guided_choice", request.guided_choice is not None),
                                       ("guided_grammar", request.guided_grammar is not None),
                                       ("response_format", request.response_format is not None
                                        and request.response_format.get("type") != "text"),
                                       ("max_tokens = 0", request.max_tokens == 0),
                                       ("a :thinking model", thinking)) if on]
    if conflicts:
        raise HTTPException(status_code=400, detail=f"beam search cannot be combined with {', '.join(conflicts)}")
    if not math.isfinite(request.length_penalty):
        raise HTTPException(status_code=400, detail="length_penalty must be a finite number")
    slots = getattr(engine, "max_choices", None)
    if slots is not None and W > slots:
        raise HTTPException(status_code=400, detail=f"beam_width = {W} exceeds the {slots} slots a worker holds")
    if not 1 <= n <= W:
        raise HTTPException(status_code=400, detail=f"n = {n} with beam search must be in 1..beam_width ({W}): it is the number of hypotheses returned")
    return {"beam_width": W, "length_penalty": float(request.length_penalty), "beam_n_best": n}


def check_beam_stops(beam: Dict[str, Any], stop_tokens) -> None:
    """400 when a beam request's distinct stop tokens do not fit beside its beams in the BEAM_K_MAX candidates of a row (both routes)."""
    if not beam:
        return
    room, have = BEAM_K_MAX - beam["beam_width"], len(set(stop_tokens))
    if have > room:
        raise HTTPException(status_code=400, detail=f"beam search: beam_width {beam['beam_width']} leaves room for {room} stop tokens, "
                            f"the request has {have}")


class ChatCompletionRequest(BaseModel):                      # api_model.py:14-62: same fields, defaults and ranges
    model: str = "rwkv-latest"
    messages: List[ChatMessage]
    stream: bool = False
    temperature: float = Field(default=DEFAULT_SAMPLING_CONFIG["temperature"], ge=0.0, le=2.0)
    top_p: float = Field(default=DEFAULT_SAMPLING_CONFIG["top_p"], ge=0.0, le=1.0)
    presence_penalty: float = Field(default=DEFAULT_SAMPLING_CONFIG["presence_penalty"], ge=0, le=2.0)
    frequency_penalty: float = Field(default=DEFAULT_SAMPLING_CONFIG["frequency_penalty"], ge=0, le=2.0)
    penalty_decay: float = Field(default=DEFAULT_SAMPLING_CONFIG["penalty_decay"], ge=0.0, le=1.0)
    max_tokens: int = Field(default=DEFAULT_SAMPLING_CONFIG["max_tokens"], ge=1)
    stop: Optional[Union[str, List[str]]] = None
    pad_zero: bool = True
    use_state_cache: bool = True
    cache_prefill: bool = True
    # log-probabilities of the generated tokens (of the raw model output: before penalties, temperature, top-p and forbidden
    # tokens) and of the top_logprobs most likely ids at each position (OpenAI's choices[0].logprobs.content)
    logprobs: bool = False
    top_logprobs: Optional[int] = Field(None, ge=0, le=20)
    # OpenAI's seed: sampled tokens draw from a generator keyed by it (reproducible for the same logits); logit_bias: token id
    # (a decimal string) -> a bias in [-100, 100] added to that token's logit
    seed: Optional[int] = Field(None, ge=-(1 << 63), lt=1 << 64)
    logit_bias: Optional[Dict[str, float]] = None
    # n choices of the prompt (prefilled once; at most a worker's slot count, else 400): choices[j] with index j, a seeded choice j
    # draws from its own Philox stream (choice 0 equals the n = 1 request with the same seed)
    n: int = Field(1, ge=1, le=128)
    # guided decoding (at most one): the content must match the regular expression / be one of the strings (extension fields, as in
    # other open servers), or OpenAI's response_format {"type": "json_schema", "json_schema": {"schema": {...}}}
    guided_regex: Optional[str] = None
    guided_choice: Optional[List[str]] = None
    guided_grammar: Optional[str] = None        # rules `name ::= body` (guided.compile_grammar); may recurse, e.g. guided.JSON_OBJECT_GRAMMAR
    response_format: Optional[Dict[str, Any]] = None
    # beam search (extension fields, as in other open servers): use_beam_search turns it on with beam_width beams (2..8, default 4)
    # and length_penalty; the request is not sampled -- temperature, top_p, seed and the penalties are accepted and ignored -- and
    # cannot stream or carry logprobs, logit_bias or a guide (400)
    use_beam_search: bool = False
    beam_width: Optional[int] = Field(None, ge=2, le=8)
    length_penalty: float = 1.0

    @model_validator(mode="after")
    def _top_logprobs_needs_logprobs(self):
        if self.top_logprobs is not None and not self.logprobs:
            raise ValueError("top_logprobs requires logprobs")
        return self

    @model_validator(mode="after")
    def _logit_bias_entries(self):
        _check_logit_bias(self.logit_bias)
        return self

    def token_bias(self) -> Dict[int, float]:
        return {int(k): float(v) for k, v in (self.logit_bias or {}).items()}


class CompletionRequest(BaseModel):
    """OpenAI's legacy completions request.  prompt: a string, a token-id list, or a list of either (one choice per prompt);
    logprobs (0..20): the log-probability of every returned token and that many alternatives; echo: the prompt comes back in front
    of the generated text, with its own logprobs when logprobs is set (max_tokens=0 then only scores the prompt).  The sampling
    fields have the chat route's defaults and ranges; n and best_of above 1 are not supported."""
    model: str = "rwkv-latest"
    prompt: Union[str, List[int], List[Union[str, List[int]]]]
    max_tokens: int = Field(default=16, ge=0)
    echo: bool = False
    logprobs: Optional[int] = Field(None, ge=0, le=20)
    stream: bool = False
    stop: Optional[Union[str, List[str]]] = None
    temperature: float = Field(default=DEFAULT_SAMPLING_CONFIG["temperature"], ge=0.0, le=2.0)
    top_p: float = Field(default=DEFAULT_SAMPLING_CONFIG["top_p"], ge=0.0, le=1.0)
    presence_penalty: float = Field(default=DEFAULT_SAMPLING_CONFIG["presence_penalty"], ge=0, le=2.0)
    frequency_penalty: float = Field(default=DEFAULT_SAMPLING_CONFIG["frequency_penalty"], ge=0, le=2.0)
    penalty_decay: float = Field(default=DEFAULT_SAMPLING_CONFIG["penalty_decay"], ge=0.0, le=1.0)
    seed: Optional[int] = Field(None, ge=-(1 << 63), lt=1 << 64)
    logit_bias: Optional[Dict[str, float]] = None
    pad_zero: bool = True
    use_state_cache: bool = True
    cache_prefill: bool = True
    n: int = 1
    best_of: Optional[int] = None
    guided_regex: Optional[str] = None
    guided_choice: Optional[List[str]] = None
    guided_grammar: Optional[str] = None        # rules `name ::= body` (guided.compile_grammar); may recurse, e.g. guided.JSON_OBJECT_GRAMMAR
    response_format: Optional[Dict[str, Any]] = None
    # beam search (extension fields, as in other open servers): use_beam_search turns it on with beam_width beams (2..8, default 4)
    # and length_penalty; the request is not sampled -- temperature, top_p, seed and the penalties are accepted and ignored -- and
    # cannot stream or carry logprobs, logit_bias or a guide (400)
    use_beam_search: bool = False
    beam_width: Optional[int] = Field(None, ge=2, le=8)
    length_penalty: float = 1.0

    @model_validator(mode="after")
    def _fields(self):
        if self.max_tokens == 0 and not self.echo:
            raise ValueError("max_tokens=0 needs echo")
        if isinstance(self.prompt, list) and len(self.prompt) == 0:
            raise ValueError("prompt is empty")
        _check_logit_bias(self.logit_bias)
        return self

    def prompts(self) -> List[Union[str, List[int]]]:
        p = self.prompt
        if isinstance(p, str) or (p and all(isinstance(x, int) for x in p)):
            return [p]
        return list(p)

    def token_bias(self) -> Dict[int, float]:
        return {int(k): float(v) for k, v in (self.logit_bias or {}).items()}


class EmbeddingRequest(BaseModel):
    """OpenAI's embeddings request.  input: a string, a list of strings, one tokenised input (a list of token ids) or a list of
    those; encoding_format "base64": the vector as little-endian float32 bytes.  Extension fields: pooling ("mean" | "last" of the
    hidden states), normalize (L2), pad_zero (the token 0 in front, as on the other routes; it is not pooled).  dimensions is refused:
    these are a language model's hidden states, and a truncated one means nothing."""
    model: str = "rwkv-latest"
    input: Union[str, List[int], List[str], List[List[int]]]
    encoding_format: Literal["float", "base64"] = "float"
    dimensions: Optional[int] = None
    pooling: str = "mean"
    normalize: bool = True
    pad_zero: bool = True

    def inputs(self) -> List[Union[str, List[int]]]:
        p = self.input
        if isinstance(p, str) or (p and all(isinstance(x, int) for x in p)):
            return [p]
        return list(p)


def legacy_top(idx2token: Dict[int, bytes], top) -> Optional[Dict[str, float]]:
    """One position's top_logprobs in the legacy format: {token string: logprob}; of ids with the same string the higher wins."""
    if top is None:
        return None
    out: Dict[str, float] = {}
    for i, v in top:
        key = idx2token.get(i, b"").decode("utf-8", errors="backslashreplace")
        if key not in out or v > out[key]:
            out[key] = v
    return out


def chat_prompt(messages: List[ChatMessage], model: str) -> Tuple[str, int]:
    """(prompt, cache_prefill_padding) of app.py:150-161: one `Role: text` paragraph per message (blank lines inside a message
    collapsed), then the assistant cue of the model variant."""
    names = {"user": "User", "assistant": "Assistant", "system": "System"}
    parts = [f"{names.get(m.role, m.role)}: {re.sub(chr(10) + '+', chr(10), (m.content or '').strip())}" for m in messages]
    variant = model.split(":")
    cue, pad = ("Assistant:<think>", 3) if "thinking" in variant else (("Assistant:", 0) if "no-thinking" in variant else ("Assistant:<think>\n</think>", 7))
    return "\n\n".join(parts + [cue]), pad


def logprob_entry(idx2token: Dict[int, bytes], tok: int, lp: Dict[str, Any]) -> Dict[str, Any]:
    """One element of OpenAI's logprobs.content: the vocabulary entry's bytes, their UTF-8 text ("" / [] for an id the vocabulary
    file does not define), the token's log-probability and its top alternatives."""
    def one(i, logprob):
        b = idx2token.get(i, b"")
        return {"token": b.decode("utf-8", errors="backslashreplace"), "logprob": logprob, "bytes": list(b)}

    return dict(one(tok, lp["logprob"]), top_logprobs=[one(i, v) for i, v in lp["top_logprobs"]])


class ThinkSplitter:
    """Splits the generated text into ("content" | "reasoning_content", piece) runs: `<think>` opens the reasoning part,
    `</think>` closes it, and a blank line in the content part ends the answer (later text is dropped) -- the rule set
    TRIE_THINK_NO_TRIGGER of streaming_string_parser.py:176-182, markers not echoed.  A marker split over several pieces is held
    back until it is complete or ruled out."""
    MARKS = {"content": (("<think>", "reasoning_content"), ("\n\n", "end")), "reasoning_content": (("</think>", "content"),), "end": ()}

    def __init__(self):
        self.state, self.held = "content", ""

    def feed(self, text: str) -> List[Tuple[str, str]]:
        out: List[Tuple[str, str]] = []
        buf = self.held + text
        self.held = ""
        while buf:
            marks = self.MARKS[self.state]
            hits = [(buf.find(m), m, nxt) for m, nxt in marks if m in buf]
            if hits:
                at, m, nxt = min(hits)
                if at:
                    out.append((buf[:at], self.state))
                if nxt == "end":
                    out.append((m, nxt))
                buf, self.state = buf[at + len(m):], nxt
                continue
            keep = max((k for m, _ in marks for k in range(1, len(m)) if buf.endswith(m[:k])), default=0)   # a marker may be arriving
            if len(buf) > keep:
                out.append((buf[:len(buf) - keep], self.state))
            self.held = buf[len(buf) - keep:] if keep else ""
            break
        merged: List[Tuple[str, str]] = []
        for piece, st in out:
            if merged and merged[-1][1] == st:
                merged[-1] = (merged[-1][0] + piece, st)
            else:
                merged.append((piece, st))
        return merged


def create_app(engine, state_cache: Optional[SimpleStateCache] = None, state_cache_size: int = 50, model_ids=None) -> FastAPI:
    """The FastAPI application over an INITIALISED engine.  state_cache: default a SimpleStateCache of state_cache_size prefixes
    (over engine.state_arena when the engine has one: prefix states stay in the workers' HBM); 0 disables caching."""
    app = FastAPI(title="RWKV OpenAI Compatible API", version="1.0.0")
    if state_cache is None and state_cache_size > 0:
        arena = getattr(engine, "state_arena", None)
        state_cache = SimpleStateCache(state_cache_size, arena=arena if (arena is not None and arena.capacity >= state_cache_size) else None)
    created = int(time.time())
    models = [{"id": i, "object": "model", "created": created, "owned_by": "chirrup"}
              for i in (model_ids or ("rwkv-latest", "rwkv-latest:thinking", "rwkv-latest:no-thinking"))]
    app.state.engine, app.state.state_cache = engine, state_cache
    idx2token = getattr(engine.tokenizer, "idx2token", {})

    @app.get("/health")
    async def health():
        return {"status": "healthy", "timestamp": int(time.time()), "model_loaded": bool(engine.is_initialized and not engine.is_shutdown)}

    @app.get("/v1/models")
    async def list_models():
        return {"object": "list", "data": models}

    async def events_of(completion, splitter, head):
        """(kind, text) pieces of a completion; the prefix-cache hand-over happens here (app.py:285-295).  head: the prompt tokens the
        request did NOT feed because it started from a cached state.  The worker reports the tokens fed SINCE admission
        (chirrup/worker.py:662 starts `prefilled_tokens` empty, as does chirrup_amd's), and the reference files the exported state under
        those alone (app.py:295) -- after a hit that is a suffix of the real prefix: the state is never found again and the requests
        waiting for the real prefix (check_and_wait_prefill) are never woken.  Here the key is the whole prefix."""
        async for ev in completion:
            if ev[0] == "token":
                if len(ev) > 4:                                # ("token", id, text, logits or None, logprobs)
                    yield "logprobs", logprob_entry(idx2token, ev[1], ev[4])
                for piece, st in splitter.feed(ev[2]):
                    if st in ("content", "reasoning_content"):
                        yield st, piece
            elif ev[0] == "cache_prefill" and state_cache is not None:
                key = tuple(head) + tuple(ev[1]["prefilled_tokens"])
                node = state_cache.cache(key, ev[1]["state"], return_trie_node=True)
                if node is not None:
                    await state_cache.awake_hang_up_prefills(key)

    async def beam_payload(completion, head):
        """The ("beams", ...) payload of a beam-search completion; the prefix-cache hand-over as in events_of."""
        payload = None
        async for ev in completion:
            if ev[0] == "beams":
                payload = ev[1]
            elif ev[0] == "cache_prefill" and state_cache is not None:
                key = tuple(head) + tuple(ev[1]["prefilled_tokens"])
                if state_cache.cache(key, ev[1]["state"], return_trie_node=True) is not None:
                    await state_cache.awake_hang_up_prefills(key)
        if completion.error:
            raise HTTPException(status_code=500, detail=f"generation failed: {completion.error}")
        if payload is None:
            raise HTTPException(status_code=500, detail=f"beam search ended without hypotheses ({completion.task.request_status})")
        return payload

    @app.post("/v1/chat/completions")
    async def chat(request: ChatCompletionRequest):
        if not engine.is_initialized or engine.is_shutdown:
            raise HTTPException(status_code=503, detail="model not loaded")
        bias = request.token_bias()
        vocab = getattr(engine, "vocab_size", None)
        if vocab is not None and bias and max(bias) >= vocab:
            raise HTTPException(status_code=400, detail=f"logit_bias: token id {max(bias)} is outside the vocabulary (size {vocab})")
        beam = beam_arguments(engine, request, request.logprobs, thinking="thinking" in request.model.split(":"), n=request.n)
        guided = guided_arguments(engine, request, thinking="thinking" in request.model.split(":"))
        n = 1 if beam else request.n                            # (with beam search n counts hypotheses of ONE request)
        if n > 1 and n > (getattr(engine, "max_choices", None) or 1):
            raise HTTPException(status_code=400, detail=f"n = {n} exceeds the {getattr(engine, 'max_choices', None) or 1} choices a worker holds")
        try:
            prompt, pad = chat_prompt(request.messages, request.model)
            tokens = ([0] if request.pad_zero else []) + engine.tokenizer.encode(prompt)
            stops: List[int] = []
            for word in ([request.stop] if isinstance(request.stop, str) else (request.stop or [])):
                stops.extend(engine.tokenizer.encode(word))
            check_beam_stops(beam, DEFAULT_STOP_TOKENS + stops)
            rest, state, n_cached = tokens, None, 0
            if request.use_state_cache and state_cache is not None:
                rest, state, n_cached = await state_cache.check_and_wait_prefill(tokens, pad)
            kw = dict(prompt_str=prompt, prefill_tokens=rest, state=state, temperature=request.temperature,
                      top_p=request.top_p, max_tokens=request.max_tokens, presence_penalty=request.presence_penalty,
                      frequency_penalty=request.frequency_penalty, penalty_decay=request.penalty_decay,
                      stop_tokens=set(DEFAULT_STOP_TOKENS + stops),
                      cache_prefill=state_cache is not None and request.cache_prefill, cache_prefill_padding=pad,
                      **({"logprobs": True, "top_logprobs": request.top_logprobs or 0} if request.logprobs else {}),
                      **({"seed": request.seed} if request.seed is not None else {}),
                      **({"logit_bias": bias} if bias else {}), **guided, **beam)
            choices = engine.completions(n=n, **kw) if n > 1 else [engine.completion(**kw)]      # one prefill for the n choices
        except HTTPException:
            raise
        except Exception as e:                                  # noqa: BLE001 -- app.py:231
            raise HTTPException(status_code=500, detail=f"generation failed: {e}")
        if beam:
            try:
                payload = await beam_payload(choices[0], tokens[:n_cached])
            finally:
                choices[0].abort()
                if state_cache is not None and request.use_state_cache and n_cached + pad != len(tokens):
                    await state_cache.awake_hang_up_prefills(tuple(tokens[:-pad]) if pad else tuple(tokens))
            out = []
            for j, h in enumerate(payload["hypotheses"]):       # rank order; the splitter applies the route's content rules
                sp = ThinkSplitter()
                sp.feed(prompt.split("\n\n")[-1])
                parts = sp.feed(h["text"])
                out.append({"index": j, "finish_reason": h["finish_reason"],
                            "message": {"role": "assistant", "content": "".join(p for p, st in parts if st == "content"),
                                        "reasoning_content": "".join(p for p, st in parts if st == "reasoning_content")}})
            n_out = sum(len(h["token_ids"]) for h in payload["hypotheses"])
            return {"id": f"chatcmpl-{uuid.uuid4().hex}", "object": "chat.completion", "created": int(time.time()), "model": request.model,
                    "choices": out, "usage": {"prompt_tokens": len(tokens), "completion_tokens": n_out, "total_tokens": len(tokens) + n_out}}
        splitters = [ThinkSplitter() for _ in choices]
        for splitter in splitters:
            splitter.feed(prompt.split("\n\n")[-1])             # the assistant cue sets the splitter's starting part (app.py:243)
        cid, created_at = f"chatcmpl-{uuid.uuid4().hex}", int(time.time())

        def chunk(delta: Dict[str, Any], finish=None, logprobs=None, index: int = 0) -> str:
            body = {"id": cid, "object": "chat.completion.chunk", "created": created_at, "model": request.model,
                    "choices": [{"index": index, "delta": delta, "finish_reason": finish}]}
            if logprobs:
                body["choices"][0]["logprobs"] = {"content": logprobs}
            return f"data: {json.dumps(body, ensure_ascii=False)}\n\n"

        async def one(index: int, completion, splitter, q: asyncio.Queue):
            """One choice: streamed chunks with its index and its own finish chunk, or (choice object, completion tokens)."""
            content, reasoning, lps, pending = [], [], [], []
            async for st, piece in events_of(completion, splitter, tokens[:n_cached]):
                if st == "logprobs":                           # rides on the next chunk sent (a token may send none)
                    lps.append(piece)
                    pending.append(piece)
                    continue
                (content if st == "content" else reasoning).append(piece)
                if request.stream:
                    q.put_nowait(chunk({"content": piece} if st == "content" else {"content": "", "reasoning_content": piece},
                                       logprobs=pending, index=index))
                    pending = []
            if completion.error:                                # the worker refused the request: reported in-band
                raise RuntimeError(completion.error)
            if request.stream:
                if pending:
                    q.put_nowait(chunk({"content": ""}, logprobs=pending, index=index))
                q.put_nowait(chunk({}, "stop", index=index))
                return None
            choice = {"index": index, "finish_reason": "stop",
                      "message": {"role": "assistant", "content": "".join(content), "reasoning_content": "".join(reasoning)}}
            if request.logprobs:
                choice["logprobs"] = {"content": lps}
            return choice, len(completion.task.generated_tokens)

        async def produce(q: asyncio.Queue):
            try:
                results = await asyncio.gather(*[one(j, c, s, q) for j, (c, s) in enumerate(zip(choices, splitters))])
                if request.stream:
                    q.put_nowait("data: [DONE]\n\n")             # once every choice has ended
                else:
                    n_out = sum(r[1] for r in results)
                    q.put_nowait(json.dumps({"id": cid, "object": "chat.completion", "created": created_at, "model": request.model,
                                             "choices": [r[0] for r in results],
                                             "usage": {"prompt_tokens": len(tokens), "completion_tokens": n_out,
                                                       "total_tokens": len(tokens) + n_out}}, ensure_ascii=False))
            except Exception as e:                              # noqa: BLE001 -- reported in-band like the reference (app.py:297-301)
                err = json.dumps({"error": {"message": str(e), "type": "internal_error"}})
                q.put_nowait(f"data: {err}\n\ndata: [DONE]\n\n" if request.stream else err)
            q.put_nowait(None)

        async def body():
            q: asyncio.Queue = asyncio.Queue()
            task = asyncio.create_task(produce(q))
            try:
                while True:
                    try:
                        item = await asyncio.wait_for(q.get(), timeout=KEEP_ALIVE_S)
                    except asyncio.TimeoutError:
                        if request.stream:
                            yield ":\n\n"                         # SSE comment: keeps proxies from closing an idle stream (app.py:325-330)
                        continue
                    if item is None:
                        return
                    yield item
            finally:                                            # client gone or done: stop generating (every choice)
                task.cancel()
                for c in choices:
                    c.abort()
                if state_cache is not None and request.use_state_cache and n_cached + pad != len(tokens):
                    # this request was the one prefilling its prefix: if it ended without exporting it (abort, failure), the requests
                    # parked on that prefix must not wait for ever (the reference leaves them waiting) -- they look again and prefill
                    await state_cache.awake_hang_up_prefills(tuple(tokens[:-pad]) if pad else tuple(tokens))

        return StreamingResponse(body(), media_type="text/event-stream" if request.stream else "application/json", headers=_SSE_HEADERS)

    def tok_str(i: int) -> str:
        return idx2token.get(i, b"").decode("utf-8", errors="backslashreplace")

    def legacy_logprobs(entries, offset: int) -> Dict[str, Any]:
        """entries: (token id, logprob or None, top [(id, logprob)] or None) -> the legacy logprobs object; text_offset counts the
        token strings from `offset`."""
        out: Dict[str, Any] = {"tokens": [], "token_logprobs": [], "top_logprobs": [], "text_offset": []}
        for tok, lp, top in entries:
            s_ = tok_str(tok)
            out["tokens"].append(s_)
            out["token_logprobs"].append(lp)
            out["top_logprobs"].append(legacy_top(idx2token, top))
            out["text_offset"].append(offset)
            offset += len(s_)
        return out

    @app.post("/v1/completions")
    async def completions(request: CompletionRequest):
        if not engine.is_initialized or engine.is_shutdown:
            raise HTTPException(status_code=503, detail="model not loaded")
        if request.n != 1 or (request.best_of is not None and request.best_of != 1):
            raise HTTPException(status_code=400, detail="n and best_of other than 1 are not supported")
        bias = request.token_bias()
        vocab = getattr(engine, "vocab_size", None)
        if vocab is not None and bias and max(bias) >= vocab:
            raise HTTPException(status_code=400, detail=f"logit_bias: token id {max(bias)} is outside the vocabulary (size {vocab})")
        beam = beam_arguments(engine, request, request.logprobs is not None)
        guided = guided_arguments(engine, request)
        k, skip = request.logprobs, (1 if request.pad_zero else 0)      # skip: the token 0 in front is fed, not echoed
        score_prompt = request.echo and k is not None
        try:
            items = []
            for p in request.prompts():
                ids = engine.tokenizer.encode(p) if isinstance(p, str) else list(p)
                if any(not 0 <= t < (vocab if vocab is not None else 1 << 62) for t in ids):
                    raise HTTPException(status_code=400, detail="prompt: a token id is outside the vocabulary")
                toks = [0] * skip + ids
                if not toks:
                    raise HTTPException(status_code=400, detail="prompt is empty")
                text = (p if isinstance(p, str) else b"".join(idx2token.get(t, b"") for t in ids).decode("utf-8", errors="replace")
                        if idx2token else engine.tokenizer.decode(ids, utf8_errors="replace"))
                items.append((toks, text))
            stops: List[int] = []
            for word in ([request.stop] if isinstance(request.stop, str) else (request.stop or [])):
                stops.extend(engine.tokenizer.encode(word))
        except HTTPException:
            raise
        except Exception as e:                                  # noqa: BLE001
            raise HTTPException(status_code=500, detail=f"generation failed: {e}")
        check_beam_stops(beam, DEFAULT_STOP_TOKENS + stops)
        cid, created_at = f"cmpl-{uuid.uuid4().hex}", int(time.time())
        # every prompt position must be fed to be scored: no prefix-state cache lookup then (the state may still be exported)
        use_cache = state_cache is not None and request.use_state_cache and not score_prompt
        completions_: List[Any] = []
        cached: Dict[int, int] = {}                             # choice index -> prompt tokens covered by a cached state

        def sse(index: int, text: str, logprobs=None, finish=None) -> str:
            body = {"id": cid, "object": "text_completion", "created": created_at, "model": request.model,
                    "choices": [{"text": text, "index": index, "logprobs": logprobs, "finish_reason": finish}]}
            return f"data: {json.dumps(body, ensure_ascii=False)}\n\n"

        async def one(index: int, toks: List[int], text: str, q: asyncio.Queue) -> Dict[str, Any]:
            echo_text = text if request.echo else ""
            if request.max_tokens == 0 and not score_prompt:     # echo alone: nothing to compute
                if request.stream:
                    q.put_nowait(sse(index, echo_text, None, "length"))
                return {"text": echo_text, "index": index, "logprobs": None, "finish_reason": "length", "n_out": 0}
            rest, state, n_cached = toks, None, 0
            if use_cache:
                rest, state, n_cached = await state_cache.check_and_wait_prefill(toks, 0)
            cached[index] = n_cached
            comp = engine.completion(prompt_str=text, prefill_tokens=rest, state=state, temperature=request.temperature,
                                     top_p=request.top_p, max_tokens=request.max_tokens, presence_penalty=request.presence_penalty,
                                     frequency_penalty=request.frequency_penalty, penalty_decay=request.penalty_decay,
                                     stop_tokens=set(DEFAULT_STOP_TOKENS + stops),
                                     cache_prefill=state_cache is not None and request.cache_prefill, cache_prefill_padding=0,
                                     **({"logprobs": True, "top_logprobs": k} if k is not None and request.max_tokens > 0 else {}),
                                     **({"prompt_logprobs": k} if score_prompt else {}),
                                     **({"seed": request.seed} if request.seed is not None else {}),
                                     **({"logit_bias": bias} if bias else {}), **guided, **beam)
            completions_.append(comp)
            if beam:                                            # choices[index] is the best hypothesis, behind the prompt with echo
                payload = await beam_payload(comp, toks[:n_cached])
                best = payload["hypotheses"][0] if payload["hypotheses"] else {"text": "", "finish_reason": "length", "token_ids": []}
                return {"text": echo_text + best["text"], "index": index, "logprobs": None, "finish_reason": best["finish_reason"],
                        "n_out": len(best["token_ids"])}
            plp: List[Any] = [None] * len(toks)
            n_plp, gen, gen_text = 0, [], []
            sent_head = False
            if request.echo and not score_prompt and request.stream:
                q.put_nowait(sse(index, echo_text))
                sent_head = True
            async for ev in comp:
                if ev[0] == "prompt_logprobs":
                    pl = ev[1]
                    for j, (t, v, top) in enumerate(zip(pl["token_ids"], pl["logprobs"], pl["top_logprobs"])):
                        plp[pl["start"] + j] = (t, v, top)
                    n_plp = pl["start"] + len(pl["logprobs"])
                    if request.stream and n_plp == len(toks) and not sent_head:
                        q.put_nowait(sse(index, echo_text, legacy_logprobs(plp[skip:], 0)))
                        sent_head = True
                elif ev[0] == "token":
                    lp = ev[4] if len(ev) > 4 else None
                    gen.append((ev[1], lp["logprob"] if lp else None, lp["top_logprobs"] if lp else None))
                    gen_text.append(ev[2])
                    if request.stream:
                        offset = len(echo_text) + sum(len(tok_str(t)) for t, _, _ in gen[:-1])
                        q.put_nowait(sse(index, ev[2], legacy_logprobs(gen[-1:], offset) if k is not None else None))
                elif ev[0] == "cache_prefill" and state_cache is not None:
                    key = tuple(toks[:n_cached]) + tuple(ev[1]["prefilled_tokens"])
                    node = state_cache.cache(key, ev[1]["state"], return_trie_node=True)
                    if node is not None:
                        await state_cache.awake_hang_up_prefills(key)
            if comp.error:
                raise RuntimeError(comp.error)
            reason = RequestStatus.get_finished_reason(comp.task.request_status)
            finish = str(reason) if reason is not None else "stop"
            logprobs = None
            if k is not None:
                entries = ([e for e in plp[skip:]] if score_prompt else []) + gen
                logprobs = legacy_logprobs(entries, 0 if score_prompt else len(echo_text))
            if request.stream:
                q.put_nowait(sse(index, "", None, finish))
            return {"text": echo_text + "".join(gen_text), "index": index, "logprobs": logprobs, "finish_reason": finish,
                    "n_out": len(comp.task.generated_tokens)}

        async def produce(q: asyncio.Queue):
            try:
                choices = await asyncio.gather(*[one(i, toks, text, q) for i, (toks, text) in enumerate(items)])
                if request.stream:
                    q.put_nowait("data: [DONE]\n\n")
                else:
                    n_in, n_out = sum(len(t) for t, _ in items), sum(c.pop("n_out") for c in choices)
                    q.put_nowait(json.dumps({"id": cid, "object": "text_completion", "created": created_at, "model": request.model,
                                             "choices": choices,
                                             "usage": {"prompt_tokens": n_in, "completion_tokens": n_out, "total_tokens": n_in + n_out}},
                                            ensure_ascii=False))
            except Exception as e:                              # noqa: BLE001 -- reported in-band, as on the chat route
                err = json.dumps({"error": {"message": str(e), "type": "internal_error"}})
                q.put_nowait(f"data: {err}\n\ndata: [DONE]\n\n" if request.stream else err)
            q.put_nowait(None)

        async def body():
            q: asyncio.Queue = asyncio.Queue()
            task = asyncio.create_task(produce(q))
            try:
                while True:
                    try:
                        item = await asyncio.wait_for(q.get(), timeout=KEEP_ALIVE_S)
                    except asyncio.TimeoutError:
                        if request.stream:
                            yield ":\n\n"
                        continue
                    if item is None:
                        return
                    yield item
            finally:
                task.cancel()
                for c in completions_:
                    c.abort()
                if use_cache:
                    for i, n_cached in cached.items():
                        toks = items[i][0]
                        if n_cached != len(toks):
                            await state_cache.awake_hang_up_prefills(tuple(toks))

        return StreamingResponse(body(), media_type="text/event-stream" if request.stream else "application/json", headers=_SSE_HEADERS)

    @app.post("/v1/embeddings")
    async def embeddings(request: EmbeddingRequest):
        if not engine.is_initialized or engine.is_shutdown:
            raise HTTPException(status_code=503, detail="model not loaded")
        if request.dimensions is not None:
            raise HTTPException(status_code=400, detail="dimensions is not supported: the vectors are hidden states of a language "
                                "model, and a truncated one means nothing")
        if request.pooling not in EMBED_POOLINGS:
            raise HTTPException(status_code=400, detail=f"pooling: expected one of {', '.join(EMBED_POOLINGS)}")
        items = request.inputs()
        if not items:
            raise HTTPException(status_code=400, detail="input is empty")
        if len(items) > EMBEDDING_INPUTS_MAX:
            raise HTTPException(status_code=400, detail=f"input holds {len(items)} entries, at most {EMBEDDING_INPUTS_MAX} are allowed")
        vocab = getattr(engine, "vocab_size", None)
        token_lists = []
        for i, p in enumerate(items):
            try:
                ids = engine.tokenizer.encode(p) if isinstance(p, str) else list(p)
            except Exception as e:                              # noqa: BLE001
                raise HTTPException(status_code=500, detail=f"embedding failed: {e}")
            if not ids:
                raise HTTPException(status_code=400, detail=f"input {i} is empty")
            if any(not 0 <= t < (vocab if vocab is not None else 1 << 62) for t in ids):
                raise HTTPException(status_code=400, detail=f"input {i}: a token id is outside the vocabulary")
            token_lists.append(ids)
        try:                                                    # one engine request per input, spread over all workers
            futures = [engine.embed(prefill_tokens=ids, pooling=request.pooling, normalize=request.normalize, pad_zero=request.pad_zero)
                       for ids in token_lists]
        except ValueError as e:
            raise HTTPException(status_code=400, detail=str(e))
        except RuntimeError as e:
            raise HTTPException(status_code=503, detail=str(e))
        try:
            results = await asyncio.gather(*futures)
        except Exception as e:                                  # noqa: BLE001
            for f in futures:
                f.cancel()
            raise HTTPException(status_code=500, detail=f"embedding failed: {e}")
        except asyncio.CancelledError:                          # client gone: stop prefilling
            for f in futures:
                f.cancel()
            raise

        def encoded(vec):
            if request.encoding_format == "base64":
                return base64.b64encode(vec.astype("<f4").tobytes()).decode("ascii")
            return [float(v) for v in vec]

        n_in = sum(int(r["prompt_tokens"]) for r in results)
        return {"object": "list", "data": [{"object": "embedding", "index": i, "embedding": encoded(r["embedding"])}
                                           for i, r in enumerate(results)],
                "model": request.model, "usage": {"prompt_tokens": n_in, "total_tokens": n_in}}

    return app


__all__ = ["create_app", "ChatCompletionRequest", "ChatMessage", "CompletionRequest", "EmbeddingRequest", "ThinkSplitter", "chat_prompt"]
