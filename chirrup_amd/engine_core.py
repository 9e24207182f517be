"""Async engine façade over N single-GPU workers (boundary B4 of SURVEY.md section 8b).

API of the reference's chirrup/engine_core.py: ``AsyncEngineCore().init(worker_num, model_config,
batch_size)`` -> asyncio.Task that completes when every worker has loaded; ``.completion(prompt_str,
...)`` -> AsyncEngineCompletion; ``.shutdown()``; ``.iter_worker_performance()``.  One shared host
task queue, workers pull from it (replica data parallelism, worker k on GPU k); worker -> asyncio
traffic goes through ``call_soon_threadsafe`` (ThreadSafeAsyncQueue, reference :30-57).

``worker_mode="thread"`` (default) runs the workers as daemon threads like the reference, which relies on a
free-threaded interpreter for that (README.md:52).  On a GIL build the per-iteration host work of N worker threads
serialises (~1 ms each per ~7.5 ms step), so ``worker_mode="process"`` gives every worker its own process, spawned
before the engine process makes any GPU call -- same messages, same pull-based balancing, queues over
``multiprocessing`` (chirrup_amd/engine_process.py).  ``worker_mode="auto"`` picks "process" for more than one worker on
an interpreter with a GIL.
"""
import sys
import asyncio
import json
import queue
import threading
import uuid
from typing import Any, AsyncIterator, Callable, Dict, List, Optional

from .core_structure import DEFAULT_SAMPLING_CONFIG, DEFAULT_STOP_TOKENS, ModelLoadConfig, Task
from .interface import AsyncEngineCompletion

GUIDE_CACHE_SIZE = 64          # compiled guides kept by the engine, least recently used first out


def _compiled_guide(cache: Dict[Any, Any], guided_regex, guided_choice, guided_json, guided_grammar=None):
    """The ByteDFA (for guided_grammar: the StackDFA) of the one guided_* argument given (None when none is): compiled here, on the caller's side, so that a bad
    pattern raises GuideError before anything is queued; a small LRU keyed by the source spares the recompilation."""
    from .guided import GuideError, compile_choice, compile_grammar, compile_regex, schema_to_regex

    given = [k for k, v in (("guided_regex", guided_regex), ("guided_choice", guided_choice), ("guided_json", guided_json),
                              ("guided_grammar", guided_grammar)) if v is not None]
    if not given:
        return None
    if len(given) > 1 and guided_grammar is not None:
        raise GuideError(f"at most one of guided_regex, guided_choice, guided_json and guided_grammar may be given, got {' and '.join(given)}")
    if len(given) > 1:
        raise GuideError(f"at most one of guided_regex, guided_choice and guided_json may be given, got {' and '.join(given)}")
    try:
        if guided_regex is not None:
            src = ("regex", guided_regex)
        elif guided_choice is not None:
            src = ("choice", tuple(guided_choice))
        elif guided_grammar is not None:
            if not isinstance(guided_grammar, str):
                raise TypeError(f"a grammar must be a string, got {type(guided_grammar).__name__}")
            src = ("grammar", guided_grammar)
        else:
            src = ("json", json.dumps(guided_json, ensure_ascii=False))
        hash(src)
    except (TypeError, ValueError) as e:
        raise GuideError(f"{given[0]}: {e}") from None
    dfa = cache.pop(src, None)
    if dfa is None:
        if guided_regex is not None:
            dfa = compile_regex(guided_regex)
        elif guided_choice is not None:
            dfa = compile_choice(list(guided_choice))
        elif guided_grammar is not None:
            dfa = compile_grammar(guided_grammar)
        else:
            dfa = compile_regex(schema_to_regex(guided_json))
    cache[src] = dfa                                   # (re-inserted: the most recently used is last)
    while len(cache) > GUIDE_CACHE_SIZE:
        cache.pop(next(iter(cache)))
    return dfa


class ThreadSafeAsyncQueue:
    """asyncio.Queue that worker threads may put into."""

    def __init__(self, event_loop: asyncio.AbstractEventLoop, q: Optional[asyncio.Queue] = None):
        self.event_loop = event_loop
        self.queue: asyncio.Queue = q if q is not None else asyncio.Queue()

    def put_nowait(self, item):
        if self.event_loop.is_closed():
            return

        def _put(x):
            try:
                self.queue.put_nowait(x)
            except asyncio.QueueFull:
                pass                      # bounded queues carry droppable telemetry only

        try:
            self.event_loop.call_soon_threadsafe(_put, item)
        except RuntimeError:
            pass                          # loop already closed

    def empty(self) -> bool:
        return self.queue.empty()

    def get_nowait(self):
        return self.queue.get_nowait()


class AsyncEngineCore:
    LOAD_TIMEOUT_S = 300

    def __init__(self, worker_factory: Optional[Callable[..., Any]] = None, tokenizer=None, worker_mode: str = "thread",
                 worker_kwargs: Optional[Dict[str, Any]] = None, state_arena_rows: int = 0, prefix_affinity: bool = True,
                 gpu_ids: Optional[List[int]] = None, state_arena_format: Optional[str] = None):
        """worker_factory(**worker_args) -> object with .start(): defaults to chirrup_amd.worker.Worker; in process mode it is
        called INSIDE the worker process and must be picklable (a module-level function).  worker_kwargs: extra Worker
        arguments (e.g. run_ahead).  state_arena_rows (process mode): rows of the HBM prefix-state arena EVERY worker process
        builds on its GPU; ``self.state_arena`` is then the engine-side view to hand to ``SimpleStateCache(arena=...)`` -- prefix
        states never leave HBM (chirrup_amd/remote_arena.py).  prefix_affinity=False queues hits on the shared queue instead of
        the owning worker's, "avoid" on ANOTHER worker's (tests: every hit is then installed through the owner's IPC handle).  gpu_ids: device of
        worker k (default k).  state_arena_format="mxint8": those arenas keep the head states packed (HbmStateArena(wkv_format=):
        about half the bytes per row; a hit continues from the codec's round trip of the exported state)."""
        if state_arena_format not in (None, "mxint8"):
            raise ValueError("state_arena_format must be None or 'mxint8'")
        self.state_arena_format = state_arena_format
        if worker_mode not in ("thread", "process", "auto"):
            raise ValueError("worker_mode must be 'thread', 'process' or 'auto'")
        self.worker_mode = worker_mode
        self._worker_kwargs = dict(worker_kwargs or {})
        self.state_arena_rows, self.prefix_affinity, self.gpu_ids = int(state_arena_rows), prefix_affinity, gpu_ids
        self.state_arena = None                       # process mode with state_arena_rows > 0: a remote_arena.RemoteArena
        self._router = None
        self._monitor = None
        self._result_q = None
        self.workers: List[Any] = []
        self.worker_threads: List[threading.Thread] = []
        self.task_queue: "queue.Queue[Task]" = queue.Queue()
        self.event_queue: "queue.Queue[Dict[str, Any]]" = queue.Queue()
        self.worker_id_set = set()
        self.worker_event_queue: Optional[ThreadSafeAsyncQueue] = None
        self.event_loop: Optional[asyncio.AbstractEventLoop] = None
        self.is_initialized = False
        self.is_shutdown = False
        self.vocab_size = None                        # model_config.vocab_size, set by init(): completion() checks logit_bias ids
        self.max_choices = None                       # a worker's slot count (batch_size - 1), set by init(): the largest n of completions()
        self.tokenizer = tokenizer
        self._worker_factory = worker_factory
        self._guide_cache: Dict[Any, Any] = {}

    def _make_worker(self, **kw):
        kw.update(self._worker_kwargs)
        if self._worker_factory is not None:
            return self._worker_factory(**kw)
        from .worker import Worker

        return Worker(**kw)

    @staticmethod
    def _gil_enabled() -> bool:
        return getattr(sys, "_is_gil_enabled", lambda: True)()

    def _start_process_workers(self, worker_num, model_config, batch_size):
        """One process per GPU, spawned before anything in THIS process has touched a GPU (it never has to)."""
        from . import engine_process as ep

        self._result_q, mp_task_q = ep.make_queues()
        kwargs = dict(self._worker_kwargs)
        if self.state_arena_rows > 0:
            from .remote_arena import RemoteArena

            kwargs["state_arena_rows"] = self.state_arena_rows
            if self.state_arena_format is not None:
                kwargs["state_arena_format"] = self.state_arena_format
            kwargs["arena_steal"] = self.prefix_affinity != "avoid"      # ("avoid": tests -- the owner must not take its hits back)
            self.state_arena = RemoteArena(self.state_arena_rows, worker_num, self._send_arena_free)
        self._router = ep.ResultRouter(self._result_q, self.worker_event_queue, self._on_process_worker_exit, self.state_arena)
        self.workers, affinity_qs = ep.spawn_workers(worker_num, model_config, batch_size, self._worker_factory, kwargs,
                                                     self._result_q, mp_task_q, self.gpu_ids)
        self.task_queue = ep.ProcessTaskQueue(mp_task_q, self._router, affinity_qs, self.prefix_affinity)
        self._router.start()
        self._monitor = ep.LivenessMonitor(self.workers, self._router, lambda: self.is_shutdown)
        self._monitor.start()

    def _send_arena_free(self, worker_id: str, row: int) -> None:
        """RemoteArena: the cache has dropped a prefix and no hit on it is in flight -- its worker may reuse the row."""
        for w in self.workers:
            if w.worker_id == worker_id and w.is_alive():
                w.control_q.put({"type": "arena_free", "row": int(row)})

    def _on_process_worker_exit(self, worker_id: str, kind: str) -> None:
        """A worker process reported an error or ended -- by its own message (router thread), or, for a hard exit (HIP abort,
        segmentation fault, kill), through the LivenessMonitor that watches the process sentinels (its thread); the router lets one
        such call run at a time (ResultRouter._worker_gone).  Its requests are completed as
        aborted (its own loop does that when it can), and so are the queued ones when no worker is left."""
        if self.is_shutdown or self._router is None:
            return
        for task in self._router.tasks_of(worker_id):
            self._router.finish_aborted(task)
        others = [w for w in self.workers if w.worker_id != worker_id and w.is_alive()]
        if self.state_arena is not None:
            # the worker's arena went with its process (round-3 advisor finding): its rows are dead in the engine's books
            # (cache lookups drop them and the requests prefill again), the hits still queued for it complete as aborted
            # (a hit carries only the tokens behind its prefix), and the surviving workers forget their views of its memory
            self.state_arena.worker_dead(worker_id)
            for tid in self.task_queue.drain_affinity(worker_id):
                task = self._router.task(tid)
                if task is not None:
                    self._router.finish_aborted(task)
            for w in others:
                w.control_q.put({"type": "peer_dead", "worker": worker_id})
        if not others:
            for task in self._router.pending():
                self._router.finish_aborted(task)
            while True:
                try:
                    self.task_queue.get_nowait()
                except Exception:                # noqa: BLE001 -- queue.Empty
                    break

    def init(self, worker_num: int, model_config: ModelLoadConfig, batch_size: int = 32) -> "asyncio.Task":
        if self.is_initialized:
            raise RuntimeError("Workers already initialized")
        if self.is_shutdown:
            raise RuntimeError("Engine has been shutdown")
        try:
            self.event_loop = asyncio.get_running_loop()
        except RuntimeError:
            self.event_loop = asyncio.new_event_loop()
            asyncio.set_event_loop(self.event_loop)
        self.worker_event_queue = ThreadSafeAsyncQueue(self.event_loop, asyncio.Queue(maxsize=worker_num * 100))
        self.vocab_size = int(model_config.vocab_size)
        self.max_choices = int(batch_size) - 1
        self.is_initialized = True
        if self.tokenizer is None:
            from .tokenizer import TRIE_TOKENIZER

            self.tokenizer = TRIE_TOKENIZER(model_config.vocab_path)

        mode = self.worker_mode
        if mode == "auto":
            mode = "process" if (worker_num > 1 and self._gil_enabled()) else "thread"
        self.worker_mode = mode

        async def wait_loaded():
            self.worker_id_set = {f"worker_{i}" for i in range(worker_num)}
            if mode == "process":
                self._start_process_workers(worker_num, model_config, batch_size)
            for k, wid in enumerate(sorted(self.worker_id_set) if mode == "thread" else []):
                w = self._make_worker(worker_id=wid, gpu_id=[k], model_config=model_config, task_queue=self.task_queue,
                                      master_event_queue=self.event_queue, worker_event_queue=self.worker_event_queue,
                                      batch_size=batch_size)
                w.on_fatal = self._on_worker_fatal
                self.workers.append(w)
                t = threading.Thread(target=w.start, daemon=True, name=f"chirrup:{wid}")
                t.start()
                self.worker_threads.append(t)
            loaded, budget = set(), self.LOAD_TIMEOUT_S
            while len(loaded) < worker_num and budget > 0:
                try:
                    wid, kind, payload = await asyncio.wait_for(self.worker_event_queue.queue.get(), timeout=1.0)
                except asyncio.TimeoutError:
                    budget -= 1
                    continue
                if kind == "worker_error" or (kind == "worker_loaded" and payload.get("status") != "success"):
                    raise RuntimeError(f"Worker {wid} failed to load: {payload}")
                if kind == "worker_loaded":
                    loaded.add(wid)
            if len(loaded) < worker_num:
                raise RuntimeError(f"workers timed out while loading: {self.worker_id_set - loaded}")

        return asyncio.create_task(wait_loaded())

    def completion(self, prompt_str: str, prefill_tokens: Optional[List[int]] = None, state=None, priority: int = 0,
                   temperature: float = DEFAULT_SAMPLING_CONFIG["temperature"], top_p: float = DEFAULT_SAMPLING_CONFIG["top_p"],
                   top_k: int = DEFAULT_SAMPLING_CONFIG["top_k"],
                   presence_penalty: float = DEFAULT_SAMPLING_CONFIG["presence_penalty"],
                   frequency_penalty: float = DEFAULT_SAMPLING_CONFIG["frequency_penalty"],
                   penalty_decay: float = DEFAULT_SAMPLING_CONFIG["penalty_decay"],
                   stop_tokens: Optional[List[int]] = DEFAULT_STOP_TOKENS, forbidden_tokens: Optional[List[int]] = None,
                   max_tokens: Optional[int] = DEFAULT_SAMPLING_CONFIG["max_tokens"], task_id: Optional[str] = None,
                   cache_prefill: bool = False, cache_prefill_padding: int = 0,
                   return_logits: bool = False, logprobs: bool = False, top_logprobs: int = 0, seed: Optional[int] = None,
                   logit_bias: Optional[Dict[int, float]] = None, prompt_logprobs: Optional[int] = None,
                   guided_regex: Optional[str] = None, guided_choice: Optional[List[str]] = None,
                   guided_json: Optional[Dict[str, Any]] = None, beam_width: int = 0, length_penalty: float = 1.0,
                   beam_n_best: int = 1, guided_grammar: Optional[str] = None) -> AsyncEngineCompletion:
        """beam_width (2..8; 0: off): beam search (DESIGN.md "Beam search") -- the request holds beam_width slots of one worker,
        streams nothing and yields one ("beams", {"hypotheses", "prompt_tokens"}) event with its beam_n_best best hypotheses, ranked by
        cumulative_logprob / max(T, 1) ** length_penalty.  It reads the raw model output: temperature, top_p, top_k, seed and the
        penalty arguments are accepted and ignored; it excludes logprobs, return_logits, prompt_logprobs, guides, logit_bias and
        forbidden_tokens, and needs stop tokens and max_tokens > 0 (ValueError).
        guided_regex / guided_choice / guided_json / guided_grammar (at most one): the generated text must match the pattern, be one
        of the strings, be compact JSON that satisfies the schema, or be a text of the grammar (guided.compile_grammar: rules
        `name ::= body` that may refer to each other and recurse, e.g. guided.JSON_OBJECT_GRAMMAR, nesting cut at 32 calls)
        (chirrup_amd/guided.py for the subsets; GuideError, a ValueError, otherwise).  The
        request then ends "stop" exactly when its text matches; it needs stop tokens."""
        assert not (state is not None and prefill_tokens is None), "prefill_tokens cannot be None when state is not None"
        if not self.is_initialized:
            raise RuntimeError("Engine not initialized")
        if self.is_shutdown:
            raise RuntimeError("Engine has been shutdown")
        bad = [t for t in (logit_bias or {}) if isinstance(t, int) and self.vocab_size is not None and t >= self.vocab_size]
        if bad:
            raise ValueError(f"logit_bias: token id {bad[0]} is outside the vocabulary (size {self.vocab_size})")
        guide = _compiled_guide(self._guide_cache, guided_regex, guided_choice, guided_json, guided_grammar)
        if beam_width and self.max_choices is not None and beam_width > self.max_choices:
            raise ValueError(f"beam_width {beam_width} exceeds a worker's slot count ({self.max_choices})")
        if not prefill_tokens:
            prefill_tokens = self.tokenizer.encode(prompt_str)
        task_id = task_id or str(uuid.uuid4())
        abort_channel = None
        if self.worker_mode == "process":
            from .engine_process import AbortChannel

            abort_channel = AbortChannel(task_id, [w.abort_q for w in self.workers])
        return AsyncEngineCompletion(prompt_str=prompt_str, prefill_tokens=list(prefill_tokens), state=state,
                                     task_queue=self.task_queue, result_channel=ThreadSafeAsyncQueue(self.event_loop),
                                     task_id=task_id, priority=priority, temperature=temperature, task_event_queue=abort_channel,
                                     top_p=top_p, top_k=top_k, presence_penalty=presence_penalty,
                                     frequency_penalty=frequency_penalty, penalty_decay=penalty_decay,
                                     stop_tokens=stop_tokens, forbidden_tokens=forbidden_tokens, max_tokens=max_tokens,
                                     cache_prefill=cache_prefill, cache_prefill_padding=cache_prefill_padding,
                                     return_logits=return_logits, logprobs=logprobs, top_logprobs=top_logprobs, seed=seed,
                                     logit_bias=logit_bias, prompt_logprobs=prompt_logprobs, guide=guide, beam_width=beam_width,
                                     length_penalty=length_penalty, beam_n_best=beam_n_best)

    def embed(self, prompt_str: Optional[str] = None, prefill_tokens: Optional[List[int]] = None, pooling: str = "mean",
              normalize: bool = True, pad_zero: bool = True, priority: int = 0) -> "asyncio.Future":
        """The text embedding of a prompt (DESIGN.md "Embeddings"): an awaitable of {"embedding": float32 ndarray [C],
        "pooled_tokens", "prompt_tokens"}.  The binary16 ln_out rows after each prompt token, averaged ("mean") or the last one
        ("last"), L2-normalised unless normalize=False.  pad_zero feeds the token 0 in front, as the other routes do; that position
        is left out of the pool.  The request only prefills and bypasses the prefix-state cache in both directions.  ValueError
        for an empty prompt or an unknown pooling, RuntimeError when the request ends without a vector (abort, worker failure)."""
        if not self.is_initialized:
            raise RuntimeError("Engine not initialized")
        if self.is_shutdown:
            raise RuntimeError("Engine has been shutdown")
        tokens = list(prefill_tokens) if prefill_tokens is not None else self.tokenizer.encode(prompt_str or "")
        if not tokens:
            raise ValueError("embed: the prompt is empty")
        bad = [t for t in tokens if not 0 <= t < (self.vocab_size if self.vocab_size is not None else 1 << 62)]
        if bad:
            raise ValueError(f"embed: token id {bad[0]} is outside the vocabulary (size {self.vocab_size})")
        task_id = str(uuid.uuid4())
        abort_channel = None
        if self.worker_mode == "process":
            from .engine_process import AbortChannel

            abort_channel = AbortChannel(task_id, [w.abort_q for w in self.workers])
        skip = 1 if pad_zero else 0
        completion = AsyncEngineCompletion(prompt_str=prompt_str or "", prefill_tokens=[0] * skip + tokens, state=None,
                                           task_queue=self.task_queue, result_channel=ThreadSafeAsyncQueue(self.event_loop),
                                           task_id=task_id, priority=priority, task_event_queue=abort_channel, max_tokens=0,
                                           embed=pooling, embed_skip=skip, embed_normalize=bool(normalize))

        async def run():
            payload = None
            try:
                async for ev in completion:
                    if ev[0] == "embedding":
                        payload = ev[1]
            except asyncio.CancelledError:
                completion.abort()
                raise
            if payload is None:
                raise RuntimeError(f"the embedding request ended without a vector ({completion.error or completion.task.request_status})")
            return payload

        return asyncio.ensure_future(run())

    def compile_guide(self, guided_regex: Optional[str] = None, guided_choice: Optional[List[str]] = None,
                      guided_json: Optional[Dict[str, Any]] = None, guided_grammar: Optional[str] = None):
        """The compiled guide completion() would use for these arguments (None without any); GuideError for a bad one.  A front end
        calls it to refuse a request before it starts answering."""
        return _compiled_guide(self._guide_cache, guided_regex, guided_choice, guided_json, guided_grammar)

    def completions(self, prompt_str: str, prefill_tokens: Optional[List[int]] = None, n: int = 1, **kw) -> List[AsyncEngineCompletion]:
        """n parallel choices of one prompt: completion()'s keywords, one AsyncEngineCompletion per choice (index order).  Starting
        any of them submits the group once; the worker prefills the prompt once and forks the state into n slots (DESIGN.md
        "Parallel choices (n)").  Each choice is iterated and aborted on its own; a seeded choice j draws from Philox stream j, so
        choice 0 equals completion() with the same seed.  1 <= n <= a worker's slot count; n > 1 excludes prompt_logprobs and
        max_tokens=0 (ValueError).  n = 1 is completion()."""
        if isinstance(n, bool) or not isinstance(n, int) or not 1 <= n <= (self.max_choices if self.max_choices is not None else n):
            raise ValueError(f"n must be an integer in [1, {self.max_choices}] (a worker's slot count), got {n!r}")
        if n == 1:
            return [self.completion(prompt_str, prefill_tokens=prefill_tokens, **kw)]
        if kw.get("beam_width"):
            raise ValueError("n > 1 cannot be combined with beam search: beam_n_best is the number of hypotheses returned")
        if kw.get("prompt_logprobs") is not None:
            raise ValueError("n > 1 cannot be combined with prompt_logprobs")
        if kw.get("max_tokens", DEFAULT_SAMPLING_CONFIG["max_tokens"]) == 0:
            raise ValueError("n > 1 needs max_tokens > 0")
        if not prefill_tokens:
            prefill_tokens = self.tokenizer.encode(prompt_str)
        task_id = kw.pop("task_id", None) or str(uuid.uuid4())
        choices = [self.completion(prompt_str, prefill_tokens=list(prefill_tokens), task_id=task_id if j == 0 else f"{task_id}:{j}",
                                   **(kw if j == 0 else dict(kw, state=None)))       # (a cached prefix state is installed for choice 0)
                   for j in range(n)]
        submitted = []

        def start_group():
            if not submitted:
                submitted.append(True)
                self.task_queue.put_nowait(choices[0].task)      # the siblings ride with choice 0

        for j, c in enumerate(choices):
            c.task.choice_index = j
            c.group_start = start_group
        choices[0].task.siblings = [c.task for c in choices[1:]]
        choices[0].task.check_group()
        return choices

    def _on_worker_fatal(self, worker, exc) -> None:
        """Called on a dying worker's thread.  When it was the last live worker, nobody will ever pick up the
        requests still in the shared queue: complete them as aborted instead of leaving their clients waiting."""
        me = threading.current_thread()
        if any(t.is_alive() and t is not me for t in self.worker_threads):
            return
        from .core_structure import RequestStatus

        while True:
            try:
                task = self.task_queue.get_nowait()
            except Exception:                    # noqa: BLE001 -- queue.Empty
                break
            for t in [task] + task.siblings:
                t.request_status = RequestStatus.FINISHED_ABORTED
                t.output_queue.put_nowait(("task_completed", t))

    def shutdown(self) -> None:
        if self.is_shutdown:
            return
        self.is_shutdown = True
        if self.worker_mode == "process" and self._router is not None:
            if self._monitor is not None:
                self._monitor.stop()
            for w in self.workers:
                w.control_q.put({"type": "shutdown"})
                w.abort_q.put(None)
            if self.state_arena is not None:
                # two phases: every worker first drops its views of the other workers' arenas ("peers_released"), only then
                # may the owners of those arenas end (engine_process.worker_process_main)
                import time

                alive = {w.worker_id for w in self.workers if w.is_alive()}
                t_end = time.time() + 15.0
                with self._router.peers_released_cv:
                    while not alive <= self._router.peers_released and time.time() < t_end:
                        self._router.peers_released_cv.wait(timeout=0.2)
                        alive = {w.worker_id for w in self.workers if w.is_alive()}
                for w in self.workers:
                    w.control_q.put({"type": "exit"})
            for w in self.workers:
                w.process.join(timeout=10)
                if w.process.is_alive():
                    w.process.terminate()
            self._result_q.put(None)
            self._result_q.cancel_join_thread()      # a worker that died holding the queue's write lock leaves this put (and the router's
            self._router.join(timeout=5)             # read) blocked for good: neither may hold up the interpreter's exit
            return
        for _ in range(max(1, len(self.workers))):       # every worker consumes one shutdown event
            self.event_queue.put_nowait({"type": "shutdown"})
        for t in self.worker_threads:
            if t.is_alive():
                t.join(timeout=5)

    async def iter_worker_performance(self, timeout: float = 1.0) -> AsyncIterator[Dict[str, Any]]:
        if self.worker_event_queue is None:
            raise RuntimeError("Engine not initialized")
        while not self.is_shutdown:
            try:
                wid, kind, payload = await asyncio.wait_for(self.worker_event_queue.queue.get(), timeout=timeout)
            except asyncio.TimeoutError:
                continue
            if kind == "worker_performance":
                yield dict(worker_id=wid, **{k: payload[k] for k in ("avg_loop_time", "state_size", "state_offset_details",
                                                                       "task_details", "max_allocated_memory_GB")})

    def __del__(self):
        try:
            self.shutdown()
        except Exception:
            pass
