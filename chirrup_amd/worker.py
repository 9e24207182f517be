"""Continuous-batching worker for one GPU (row A10 of SURVEY.md section 8a; boundary B4).

Keeps the reference worker's protocol and scheduling semantics (chirrup/worker.py):
  * ``Worker(worker_id, gpu_id, model_config, task_queue, master_event_queue, worker_event_queue,
    batch_size).start()`` runs the loop in the calling thread until a {"type": "shutdown"} event;
  * slots are classified with ``StateCategory`` (same members / order, :86-92); decode rows and
    single-token prefill rows share one forward per iteration (:671-742), chunked prefill of at most
    ``max_forward_seq_len_per_forward`` tokens runs every ``decode_prefill_ratio`` iterations for at
    most ``max(batch_size/8, 1)`` sequences (:143, :744-776, :854-856);
  * messages: ("token_generated", (id, text[, logits])) -- (id, text, logits or None, logprobs) for a request with
    ``logprobs`` --, ("task_completed", task),
    ("beams", {"hypotheses", "prompt_tokens"}) instead of token messages for a beam-search request (DESIGN.md "Beam search"),
    ("cache_prefill", {"state", "prefilled_tokens"}) on the task's output queue (:422-434, :498-501,
    :556-558), (worker_id, "worker_loaded" | "worker_performance", {...}) on the worker event queue.

What is different is the DEVICE DISPATCH, redesigned for a 288 GB MI355X:
  * the slot table never moves.  The reference sorts slots by category with physical swaps of three
    17 MB state blocks per swap (`_switch_batch`, :304-360) so that a category is a contiguous slice;
    here every forward takes an int32 ``slot_idx`` vector and the kernels index the pool directly
    (RWKV_x070.forward_slots).  ``min_swaps_to_target_fast`` is still exported (tested API).
  * penalties + greedy sampling of all decode rows are one kernel and one D2H copy of B ids
    (ops.penalize_argmax) instead of ~8 torch kernels and B ``.item()`` syncs (:719-740); rows with
    real sampling parameters go through samplers.sample_logits_rwkv_pip_compatible.
  * prefix states exported for the cache stay in HBM by default (device clones; `state_cache_device="cpu"`
    restores the reference's host copies) -- a cache hit is then a 17-33 MB device-to-device copy.
  * RUN-AHEAD: the sampled ids never have to reach the host before the next forward.  They are scattered into a
    per-slot device vector (``last_ids``) that the next forward gathers its decode inputs from, and the penalty
    state (occurrence += 1, presence) is updated on the device from the same ids.  ``step()`` therefore launches
    forward k and only then reads and handles the ids of forward k-1 (text decode, stop / length checks, messages,
    admission): the ~1 ms of per-token host bookkeeping runs under the ~9 ms forward instead of in series with it.
    A request that turns out to have finished at k-1 has one speculative row in forward k; that row's result is
    dropped (the slot is recycled afterwards, in stream order).  ``run_ahead=False`` handles each forward's ids in
    the same ``step()`` call, like the reference's loop; both modes produce the same token streams.
"""
import math
import queue
import struct
import time
import types
from collections import deque
from enum import IntEnum, auto
from typing import Dict, List, Optional, Tuple

import torch

from . import ops
from .core_structure import LOGIT_BIAS_MAX, ModelLoadConfig, RequestStatus, Task
from .embeddings import finish as finish_embedding
from .guided import GuideError, StackDFA, token_table
from .samplers import is_greedy_row, sample_inverse_cdf, sample_logits_rwkv_pip_compatible


class StateCategory(IntEnum):
    FORWARD_ONE_DECODE = auto()
    FORWARD_ONE_PREFILL = auto()
    FORWARD_ONE_SUSPENDED = auto()
    FORWARD_SEQ = auto()
    FINISHED = auto()
    EMPTY = auto()


def min_swaps_to_target_fast(lst, elements):
    """Partition ``lst`` in place so that equal categories are contiguous in the order of
    ``elements``; returns (swaps, offsets) like chirrup/worker.py:43-78.  This worker does not need
    the swaps (it uses slot indices) but the function is part of the reference's tested surface."""
    swaps: List[Tuple[int, int]] = []
    offsets: List[Tuple[int, int]] = []
    lo = 0
    for cat in elements:
        here = [i for i in range(lo, len(lst)) if lst[i] == cat]
        hi = lo + len(here)
        offsets.append((lo, hi))
        inside = set(here)
        holes = [i for i in range(lo, hi) if i not in inside]
        for hole, src in zip(holes, [i for i in here if i >= hi]):
            swaps.append((hole, src))
            lst[hole], lst[src] = lst[src], lst[hole]
        lo = hi
    return swaps, offsets


def _empty_slot() -> dict:
    # feedback: the slot's next decode input is last_ids[slot] on the device.  Prompt logprobs (task.prompt_logprobs set):
    # plp_prompt = the tokens as admitted, plp_next = index of the next one to feed, plp_sent = positions already sent.
    # Parallel choices: siblings = [(slot, task)] of the choices waiting suspended for this slot's prefill (until the fork); orphan:
    # choice 0 has aborted and the slot prefills on for its live siblings only.  emb_fed: prompt positions an embedding request has fed
    # beam: (group, position) of a slot that holds one beam of a beam-search request, from the fork to the request's end
    return {"beam": None, "emb_fed": 0, "task": None, "is_prefilling": None, "new_token": None, "next_input_token": None,
            "state_category": StateCategory.EMPTY, "prefilled_tokens": [], "prefill_cached": False,
            "feedback": False, "plp_prompt": None, "plp_next": 0, "plp_sent": 0, "siblings": None, "orphan": False}


class _NullSink:
    """The output queue of the internal tasks that hold the further slots of a beam-search request: nobody reads their messages."""

    def put_nowait(self, msg):
        pass


class GuidePool:
    """The guides of one worker (DESIGN.md "Guided decoding"): every guide in use or recently used is a contiguous range of rows of
    ``next`` int32 [P, 256] (absolute rows, -1 dead) and ``allow`` int32 [P, V/32] (uint32 bitmap words: the tokens a state allows);
    ``state`` int32 [slots] holds each slot's current row, -1 for an unconstrained slot.  A guide is cached under (guide.key, its
    sorted stop tokens) -- the stop tokens decide the bitmaps -- with a reference count; when a new guide finds no free range, the
    least recently used guides nobody holds are dropped until it fits.  The token byte table is uploaded once."""

    def __init__(self, rows: int, n_slots: int, V: int, device, idx2token):
        if V % 64:
            raise GuideError(f"guided decoding needs a vocabulary size that is a multiple of 64, got {V}")
        if not idx2token:
            raise GuideError("guided decoding needs the tokenizer's byte table (idx2token)")
        off, data = token_table(idx2token, V)
        self.P, self.V, self.device = int(rows), V, device
        self.tok_off, self.tok_bytes = torch.from_numpy(off).to(device), torch.from_numpy(data).to(device)
        self.next = torch.full((self.P, 256), -1, dtype=torch.int32, device=device)
        self.allow = torch.zeros((self.P, V // 32), dtype=torch.int32, device=device)
        self.state = torch.full((n_slots,), -1, dtype=torch.int32, device=device)
        self.entries: Dict[tuple, dict] = {}          # key -> {"row0", "S", "refs", "tick"}
        self._tick = 0
        self.builds = 0                               # guides built (a cache hit builds nothing)

    def _place(self, S: int) -> Optional[int]:
        at = 0
        for e in sorted(self.entries.values(), key=lambda e: e["row0"]):      # first fit among the gaps
            if e["row0"] - at >= S:
                return at
            at = e["row0"] + e["S"]
        return at if self.P - at >= S else None

    def acquire(self, guide, stop_tokens) -> Tuple[tuple, int]:
        """(cache key, start row) of the guide for a request with these stop tokens, built when it is new; the caller holds one
        reference until release(key).  GuideError when it cannot be placed or the vocabulary cannot realise it."""
        key = (guide.key, tuple(sorted(int(t) for t in stop_tokens)))
        self._tick += 1
        e = self.entries.get(key)
        if e is not None:
            e["refs"] += 1
            e["tick"] = self._tick
            return key, e["row0"]
        S = int(guide.next.shape[0])
        row0 = self._place(S)
        while row0 is None:
            idle = [k for k, v in self.entries.items() if v["refs"] == 0]
            if not idle:
                raise GuideError(f"the guide pool ({self.P} rows) has no room for a guide of {S} states: "
                                 f"{sum(v['S'] for v in self.entries.values())} rows are held by running requests")
            del self.entries[min(idle, key=lambda k: self.entries[k]["tick"])]
            row0 = self._place(S)
        import numpy as np

        # stream-ordered writes: rows of a dropped guide may still be read by a run-ahead row in flight, which runs first
        self.next[row0:row0 + S] = torch.from_numpy(np.where(guide.next >= 0, guide.next + np.int32(row0), np.int32(-1)).astype(np.int32)).to(self.device)
        accept = torch.from_numpy(np.ascontiguousarray(guide.accept).astype(np.uint8)).to(self.device)
        special = torch.tensor(key[1], dtype=torch.int32).to(self.device)
        ops.guide_build(S, row0, self.next, self.tok_off, self.tok_bytes, special, accept, self.allow)
        self.builds += 1
        # the one host synchronisation of the feature, once per new guide: a state that allows no token would leave its row with
        # nothing to sample (the vocabulary cannot spell what the pattern asks for there)
        empty = (self.allow[row0:row0 + S] == 0).all(dim=1)
        if bool(empty.any()):
            raise GuideError(f"the vocabulary cannot realise the pattern: state {int(empty.nonzero()[0])} of its automaton allows no token")
        self.entries[key] = {"row0": row0, "S": S, "refs": 1, "tick": self._tick}
        return key, row0

    def release(self, key) -> None:
        e = self.entries.get(key)
        if e is not None and e["refs"] > 0:
            e["refs"] -= 1


class GrammarPool:
    """The grammar guides of one worker (DESIGN.md "Grammar-guided decoding"): a pool of its own beside GuidePool, with the same
    placement, cache key (guide.key, the sorted stop tokens), reference counts and LRU eviction.  A guide is a contiguous range of
    rows of ``next`` int32 [P, 256], ``meta`` int32 [P, 8] and the bitmaps ``allow`` / ``maybe`` int32 [P, V/32] (layout:
    include/chirrup_amd.h); ``state`` int32 [slots] is each slot's current row (-1: no grammar) and ``stack`` int64 [slots, 4] its
    call stack."""

    def __init__(self, rows: int, n_slots: int, V: int, device, idx2token):
        if V % 64:
            raise GuideError(f"guided decoding needs a vocabulary size that is a multiple of 64, got {V}")
        if not idx2token:
            raise GuideError("guided decoding needs the tokenizer's byte table (idx2token)")
        off, data = token_table(idx2token, V)
        self.single = {b[0] for i, b in idx2token.items() if 0 <= i < V and len(b) == 1}     # the bytes that are tokens by themselves
        self.P, self.V, self.device = int(rows), V, device
        self.tok_off, self.tok_bytes = torch.from_numpy(off).to(device), torch.from_numpy(data).to(device)
        self.next = torch.full((self.P, 256), -1, dtype=torch.int32, device=device)
        self.meta = torch.full((self.P, ops.GRAMMAR_META_WORDS), -1, dtype=torch.int32, device=device)
        self.allow = torch.zeros((self.P, V // 32), dtype=torch.int32, device=device)
        self.maybe = torch.zeros((self.P, V // 32), dtype=torch.int32, device=device)
        self.state = torch.full((n_slots,), -1, dtype=torch.int32, device=device)
        self.stack = torch.zeros((n_slots, 4), dtype=torch.int64, device=device)
        self.entries: Dict[tuple, dict] = {}          # key -> {"row0", "S" (rows held), "refs", "tick"}
        self._tick = 0
        self.builds = 0

    _place = GuidePool._place
    release = GuidePool.release

    def acquire(self, guide, stop_tokens) -> Tuple[tuple, int]:
        """(cache key, start row) of the grammar for a request with these stop tokens, built when it is new; the caller holds one
        reference until release(key).  GuideError when it cannot be placed or the vocabulary cannot spell it: with every byte
        that labels an edge a token by itself, and the compiler's depth accounting, a guided row always has an allowed token."""
        key = (guide.key, tuple(sorted(int(t) for t in stop_tokens)))
        self._tick += 1
        e = self.entries.get(key)
        if e is not None:
            e["refs"] += 1
            e["tick"] = self._tick
            return key, e["row0"]
        missing = [b for b in guide.edge_bytes() if b not in self.single]
        if missing:
            raise GuideError(f"the vocabulary cannot realise the grammar: the byte {bytes(missing[:1])!r} labels an edge of its automaton "
                             f"and is no token by itself ({len(missing)} such bytes)")
        R = ops.grammar_guide_rows(guide, len(key[1]))
        row0 = self._place(R)
        while row0 is None:
            idle = [k for k, v in self.entries.items() if v["refs"] == 0]
            if not idle:
                raise GuideError(f"the grammar pool ({self.P} rows) has no room for a guide of {R} rows: "
                                 f"{sum(v['S'] for v in self.entries.values())} rows are held by running requests")
            del self.entries[min(idle, key=lambda k: self.entries[k]["tick"])]
            row0 = self._place(R)
        # stream-ordered writes: rows of a dropped guide may still be read by a run-ahead row in flight, which runs first
        nxt, meta = ops.grammar_guide_tables(guide, row0, key[1])
        self.next[row0:row0 + R] = torch.from_numpy(nxt).to(self.device)
        self.meta[row0:row0 + R] = torch.from_numpy(meta).to(self.device)
        special = torch.tensor(key[1], dtype=torch.int32).to(self.device)
        ops.grammar_build(guide.n_states, row0, self.next, self.meta, self.tok_off, self.tok_bytes, special, self.allow, self.maybe)
        self.builds += 1
        self.entries[key] = {"row0": row0, "S": R, "refs": 1, "tick": self._tick}
        return key, row0


class Worker:
    def __init__(self, worker_id: str, gpu_id: List[int], model_config: ModelLoadConfig, task_queue: queue.Queue,
                 master_event_queue: queue.Queue, worker_event_queue: Optional[queue.Queue], batch_size: int = 32,
                 model=None, tokenizer=None, penalize_argmax=None, state_cache_device=None, run_ahead: bool = True,
                 state_arena=None, state_arena_rows: int = 0, peer_arenas=None, guide_pool_rows: int = 16384,
                 grammar_pool_rows: int = 2048, state_arena_format: Optional[str] = None):
        self.worker_id, self.gpu_id, self.model_config = worker_id, gpu_id, model_config
        self.task_queue, self.master_event_queue, self.worker_event_queue = task_queue, master_event_queue, worker_event_queue
        self.real_state_size = batch_size
        self.max_batch_size = batch_size - 1          # the reference keeps one scratch slot; kept for parity of capacity
        self.max_prefill_count = max(int(batch_size * 0.125), 1)
        self.state_slot: Dict[int, dict] = {i: _empty_slot() for i in range(self.max_batch_size)}
        self.model, self.tokenizer = model, tokenizer   # may be injected (tests use a fake backend)
        self._slot_cache: Dict[tuple, torch.Tensor] = {}
        self._max_mem_gb = None
        self._penalize_argmax = penalize_argmax if penalize_argmax is not None else ops.penalize_argmax
        self._sample_topp = ops.sample_topp if penalize_argmax is None else None     # fake backends use the torch sampler
        self._commit_kernel = ops.commit_sampled if penalize_argmax is None else None  # ... and torch ops for the commit
        self.batch_state = None
        # where exported prefix states live: None = the pool's own device (HBM-resident prefix cache:
        # 17-33 MB device-to-device copies instead of two PCIe transfers per cache hit); "cpu" = the
        # reference's behaviour (worker.py:427-429)
        self.state_cache_device = state_cache_device
        # an HbmStateArena on this worker's device: prefix states are exported straight into a free arena row (one copy)
        # and travel as ArenaRef handles; without it they are device clones (or host copies, state_cache_device="cpu")
        self.state_arena = state_arena
        # process mode: build an arena of this many rows on this worker's own device (after the model has loaded) and publish it
        # to the other worker processes (remote_arena.PeerArenas): prefix states then never leave HBM
        self.state_arena_rows, self.peer_arenas = int(state_arena_rows), peer_arenas
        # how that arena keeps state[1]: None = binary16 as in the slot table, "mxint8" = packed (HbmStateArena(wkv_format=))
        self.state_arena_format = state_arena_format
        self._pending_installs = []                   # (event, task id): copies out of ANOTHER worker's arena still in flight
        self.run_ahead = run_ahead
        self.on_fatal = None                          # callable(worker, exception), set by the engine
        self._inflight = None                         # the forward whose sampled ids the host has not handled yet
        self.no_penalty_token_ids = {33, 10, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58}
        self.min_forward_seq_len = 10
        self.max_forward_seq_len_per_forward = 100
        self.seq_forward_count_down = 0
        self.decode_prefill_ratio = 5
        # NOT the reference's policy (off by default): while fewer than half of the slots are decoding, run a prefill chunk in
        # EVERY iteration instead of every decode_prefill_ratio-th -- a batch that arrives at once reaches full width after
        # n_chunks iterations instead of 5 x n_chunks (bench.py --serving-fill-first)
        self.prefill_when_underfilled = False
        self.shutdown_flag = False
        self.loop_time_recorder = deque(maxlen=10)
        self.iterations = 0
        self._held = None                             # a group of parallel choices pulled before n slots were free
        self._groups: List[Tuple[int, Task]] = []     # (slot, choice-0 task) of the admitted groups that have not forked yet
        # guided decoding: the pool (rows of automaton states: 8 KiB + 1 KiB per row at V = 65536) is allocated when the first guided
        # request arrives; _guide_refs: id(task) -> (cache key, start row) of the admitted guided requests; _guided: the slots whose
        # guide_state entry is not -1 (host mirror, like _bias_n)
        self.guide_pool_rows = int(guide_pool_rows)
        self._guides: Optional[GuidePool] = None
        self._guide_refs: Dict[int, tuple] = {}
        self._guided = [False] * batch_size
        # grammar guides (guided.StackDFA) have a pool of their own, allocated when the first grammar request arrives; _grammared: the
        # slots whose row in it is not -1.  A slot is in at most one of _guided / _grammared
        self.grammar_pool_rows = int(grammar_pool_rows)
        self._grammars: Optional[GrammarPool] = None
        self._grammared = [False] * batch_size
        self._grammar_resets: Dict[int, int] = {}     # slot -> start row (or -1) written since the last forward: one reset launch
        # text embeddings (DESIGN.md "Embeddings"): per-slot accumulators (sum fp32 [n, C], last row fp16 [n, C], rows int32 [n]) that
        # ops.pool_rows fills chunk by chunk, allocated when the first embedding request arrives; _emb_host: two sets of pinned host
        # copies (the loop runs one forward ahead of the host), _emb_downloads picks the set
        self._emb = None
        self._emb_host = None
        self._emb_downloads = 0
        # beam search (DESIGN.md "Beam search"): beam_scores fp32 [slots] is the device's score table; _beam_host: two pinned sets of
        # the per-step outputs (the loop runs one forward ahead of the host); beam_trace: every record also carries the step's
        # downloaded candidate tables (tests replay the contract from them)
        self.beam_trace = False
        self._beam_host = None
        self._beam_tables: Dict[tuple, tuple] = {}
        self._beam_live = 0                           # forked beam groups that have not ended: 0 keeps every step off the beam path

    # ------------------------------------------------------------------ set-up
    def _load_model(self):
        from .rwkv7 import RWKV_x070, model_args
        from .tokenizer import TRIE_TOKENIZER

        if self.model is None:
            self.model = RWKV_x070(model_args(self.model_config.model_path, self.model_config.vocab_size,
                                              self.model_config.head_size),
                                   ffn_dtype=(torch.int8 if self.model_config.dtype == torch.int8 else
                                              "mxfp4" if self.model_config.dtype == "mxfp4" else torch.float16),
                                   att_dtype=torch.int8 if getattr(self.model_config, "att_dtype", None) == torch.int8 else torch.float16)
        if self.tokenizer is None:
            self.tokenizer = TRIE_TOKENIZER(self.model_config.vocab_path)
        self._post({"status": "success", "worker_id": self.worker_id, "gpu_id": self.gpu_id,
                    "model_path": self.model_config.model_path}, "worker_loaded")

    def _post(self, payload, kind):
        if self.worker_event_queue is not None:
            try:
                self.worker_event_queue.put_nowait((self.worker_id, kind, payload))
            except queue.Full:      # performance messages are droppable (engine_core.py:42-47)
                pass

    def _init_worker(self):
        if self.gpu_id and torch.cuda.is_available():
            torch.cuda.set_device(self.gpu_id[0])
        self._load_model()
        n, V = self.real_state_size, self.model_config.vocab_size
        self.batch_state = self.model.generate_zero_state(n)
        dev = self.batch_state[0].device
        self.device = dev
        f32 = dict(dtype=torch.float32, device=dev)
        self.occurrence = torch.zeros((n, V), **f32)
        self.alpha_presence_vector = torch.zeros((n, V), **f32)
        self.temperature_tensor = torch.zeros((n, 1), dtype=torch.float16, device=dev)
        self.top_p_tensor = torch.zeros((n, 1), dtype=torch.float16, device=dev)
        self.top_k_tensor = torch.zeros((n, 1), dtype=torch.int32, device=dev)
        self.frequency_penalty_tensor = torch.zeros((n, 1), dtype=torch.float16, device=dev)
        self.penalty_decay_tensor = torch.zeros((n, 1), dtype=torch.float16, device=dev)
        self.presence_penalty_tensor = torch.zeros((n, 1), **f32)
        self._greedy = [True] * n
        # per-request seeds (ops.seeded_uniform): the Philox key and each slot's draw counter; host mirrors say which slots hold a
        # seed / a logit_bias list, so that steps and installs of requests without either touch none of these tables
        self.seeds = torch.zeros((n,), dtype=torch.int64, device=dev)
        self.seeded = torch.zeros((n,), dtype=torch.int32, device=dev)
        self.counters = torch.zeros((n,), dtype=torch.int32, device=dev)
        self._seeded = [False] * n
        # logit_bias lists (ops.apply_logit_bias): ids / values [n, LOGIT_BIAS_MAX], entries per slot
        self.bias_ids = torch.zeros((n, LOGIT_BIAS_MAX), dtype=torch.int32, device=dev)
        self.bias_values = torch.zeros((n, LOGIT_BIAS_MAX), **f32)
        self.bias_counts = torch.zeros((n,), dtype=torch.int32, device=dev)
        self._bias_n = [0] * n
        # device-side feedback of the sampled ids (run-ahead): next decode inputs and the penalty bookkeeping
        self.last_ids = torch.zeros((n,), dtype=torch.int32, device=dev)
        self.beam_scores = torch.zeros((n,), **f32)
        self.penalty_weight = torch.ones((V,), **f32)           # occurrence increment per token id (worker.py:531)
        self.penalty_weight[[t for t in self.no_penalty_token_ids if t < V]] = 0.0
        self._ids_host = ([torch.zeros((n + 1,), dtype=torch.int32).pin_memory() for _ in range(2)]     # (+ 1: the launch-status word)
                          if dev.type == "cuda" else None)
        self._launches = 0
        self._lp_host = None                          # pinned [2] x (lp, ids) of the logprob rows, allocated when a request first asks
        # the ids each slot has sampled (ops.PenaltyLists): the penalty step then touches those entries of the dense tables only
        self._pen_lists = (ops.PenaltyLists(n, V, dev) if (self._commit_kernel is not None and dev.type == "cuda" and V % 32 == 0
                                                           and self._penalize_argmax is ops.penalize_argmax) else None)
        if self.state_arena is None and self.state_arena_rows > 0:
            from .state_cache import HbmStateArena

            s0, s1 = self.batch_state[0], self.batch_state[1]
            self.state_arena = HbmStateArena(s0.shape[0], s0.shape[3], self.state_arena_rows, dev, dtype=s0.dtype,
                                             wkv_shape=s1.shape[2:], wkv_dtype=s1.dtype, wkv_format=self.state_arena_format)
            if hasattr(self.task_queue, "arena"):
                self.task_queue.arena = self.state_arena          # exports into it leave this process as row addresses
            if self.peer_arenas is not None:
                self.peer_arenas.publish(self.state_arena)
        # decode-step HIP graphs per batch bucket (captured lazily); slot n-1 is the parking slot
        self._graphs = {}
        self.use_graph = bool(getattr(self.model, "fused", False)) and self.device.type == "cuda"

    # ------------------------------------------------------------------ per-slot bookkeeping (host only)
    def _process_events(self) -> bool:
        while True:
            try:
                ev = self.master_event_queue.get_nowait()
            except queue.Empty:
                return False
            if ev.get("type") == "shutdown":
                self.shutdown_flag = True
                return True
            if ev.get("type") == "arena_free" and self.state_arena is not None:
                self.state_arena.release(int(ev["row"]))       # the engine's cache dropped the prefix: the row may be reused
            if ev.get("type") == "peer_dead" and self.peer_arenas is not None:
                self.peer_arenas.forget(ev["worker"])          # another worker process has ended: its arena is gone

    @staticmethod
    def _is_task_aborted(td) -> bool:
        q = td["task"].task_event_queue
        if q.empty():                       # the common case, without the cost of raising queue.Empty
            return False
        try:
            kind, _ = q.get_nowait()
            return kind == "abort"
        except queue.Empty:
            return False

    def _export_state(self, slot: int):
        """[state0[:, :, [s]], state1[:, [s]], state2[[s]]] on the CPU (worker.py:426-430)."""
        s0, s1, s2 = self.batch_state
        if self.state_arena is not None and self.state_arena.free_rows > 0:
            return self.state_arena.export_slot(self.batch_state, slot)      # slot -> arena row, one strided copy per tensor
        parts = [s0[:, :, [slot], :], s1[:, [slot], :, :], s2[[slot]]]      # advanced indexing: fresh copies
        if self.state_cache_device is None:
            return parts
        return [p.to(self.state_cache_device, non_blocking=True) for p in parts]

    def _maybe_cache_prefill(self, td, slot: int):
        t: Task = td["task"]
        if t.cache_prefill and not td["prefill_cached"] and len(t.prefill_tokens) == max(t.cache_prefill_padding - 1, 0):
            t.output_queue.put_nowait(("cache_prefill", {"state": self._export_state(slot),
                                                         "prefilled_tokens": tuple(td["prefilled_tokens"])}))
            td["prefill_cached"] = True
            return True
        return False

    def _handle_forward_seq(self, td, slot: int):
        t: Task = td["task"]
        if t.embed is not None:                         # an embedding is prefilled by chunks only, whatever is left of it
            return
        if self._maybe_cache_prefill(td, slot):
            td["state_category"] = StateCategory.FORWARD_ONE_PREFILL
        if len(t.prefill_tokens) == 0:
            td["state_category"], td["is_prefilling"] = StateCategory.FORWARD_ONE_DECODE, False
            self._maybe_end_scoring(td)
        elif len(t.prefill_tokens) < self.min_forward_seq_len:
            td["state_category"] = StateCategory.FORWARD_ONE_PREFILL

    def _handle_forward_one_prefill_phase(self, td, slot: int):
        t: Task = td["task"]
        td["prefilled_tokens"].append(td["next_input_token"])
        td["next_input_token"] = t.prefill_tokens.pop(0)
        if len(t.prefill_tokens) == 0:
            td["is_prefilling"], td["state_category"] = False, StateCategory.FORWARD_ONE_DECODE
        self._maybe_cache_prefill(td, slot)
        if len(t.prefill_tokens) == 0:
            self._maybe_end_scoring(td)

    @staticmethod
    def _scoring_only(t: Task) -> bool:
        return t.prompt_logprobs is not None and t.max_tokens == 0

    def _maybe_end_scoring(self, td):
        """A scoring-only request (prompt_logprobs, max_tokens=0) whose next input is its last prompt token: that token is never
        fed.  It ends (length) now if every prompt position has been sent, else it waits suspended for the forward in flight."""
        t: Task = td["task"]
        if not self._scoring_only(t):
            return
        if td["plp_sent"] >= len(td["plp_prompt"]):
            t.request_status = RequestStatus.FINISHED_LENGTH_CAPPED
        else:
            td["state_category"] = StateCategory.FORWARD_ONE_SUSPENDED

    def _handle_forward_one_decode_phase(self, td, tok: int, raw_logits=None, logprobs=None):
        """One sampled token of a live request (chirrup/worker.py:503-560): stop / length checks, text, message.
        The penalty state was already advanced on the device when the token was sampled.  logprobs: {"logprob", "top_logprobs"}
        of the token (requests with ``logprobs``)."""
        t: Task = td["task"]
        td["new_token"] = tok
        if tok in t.stop_tokens:
            t.request_status = RequestStatus.FINISHED_STOPPED
            return
        try:
            text = self.tokenizer.decode([tok], utf8_errors="ignore")
        except KeyError:                 # an id the vocabulary file does not define (the model's vocab is padded)
            text = ""
        t.generated_tokens.append(tok)
        t.decoded_texts.append(text)
        if t.logprobs:
            raw = raw_logits.detach().cpu() if (t.return_logits and raw_logits is not None) else None
            t.output_queue.put_nowait(("token_generated", (tok, text, raw, logprobs)))
        elif t.return_logits and raw_logits is not None:
            t.output_queue.put_nowait(("token_generated", (tok, text, raw_logits.detach().cpu())))
        else:
            t.output_queue.put_nowait(("token_generated", (tok, text)))
        if len(t.generated_tokens) >= t.max_tokens:
            t.request_status = RequestStatus.FINISHED_LENGTH_CAPPED
            return
        td["next_input_token"] = tok

    def _commit_sampled(self, ids: torch.Tensor, didx: torch.Tensor, status_out=None):
        """Device-side consequences of sampling `ids` for the slots `didx`: the next decode input and the
        repetition-penalty state (worker.py:527-535: occurrence += 1 except for the no-penalty ids, presence).
        status_out: the element behind the ids that receives the device's sticky launch-status word in the same launch."""
        if self._commit_kernel is not None:                # one launch instead of ~12 eager ones behind every decode step
            self._commit_kernel(ids, didx, self.last_ids, self.occurrence, self.penalty_weight, self.alpha_presence_vector,
                                self.presence_penalty_tensor, status_out=status_out, **({"lists": self._pen_lists} if self._pen_lists is not None else {}))
            return
        dl, il = didx.long(), ids.long()
        self.last_ids.index_copy_(0, dl, ids)
        self.occurrence.index_put_((dl, il), self.penalty_weight[il], accumulate=True)
        self.alpha_presence_vector[dl, il] = self.presence_penalty_tensor[dl, 0]

    def _handle_results(self, rec):
        """Host half of a forward: read its sampled ids and run the per-token bookkeeping.  Rows whose request
        is gone (finished or aborted while this forward was in flight) are dropped."""
        if rec is None:
            return
        if isinstance(rec, list):                           # the records of one step: its single-token forward, then its chunk
            for r in rec:
                self._handle_results(r)
            return
        if rec["event"] is not None:
            rec["event"].synchronize()
        if rec.get("plp") is not None:
            self._handle_prompt_logprobs(rec["plp"])
        if rec.get("emb") is not None:
            self._handle_embeddings(*rec["emb"])
        n_rows = len(rec["rows"])
        if n_rows == 0:
            return
        host_ids = rec["ids"][: n_rows + (1 if rec.get("status") else 0)].tolist()        # ONE device->host copy for the whole batch
        if rec.get("status") and host_ids[n_rows] != 0:
            # the time-mix launch's bounded in-launch waits (include/chirrup_amd.h: rwkv7_tmix_gemms): a wait that gave up left the LoRA
            # outputs of a step at or before this one undefined -- never seen on a GPU this process has to itself.  The sticky status
            # word arrives behind every step's ids, so the step that gave up is fatal BEFORE any of its tokens is sent to a client
            # (round 3 looked at a word every replay had zeroed, every 256 iterations).
            raise RuntimeError(f"a time-mix launch gave up waiting for its own workgroups (status word {host_ids[n_rows]}): results are undefined")
        lp = rec.get("lp")
        if lp is not None:                                  # one copy each for the logprob rows' values and top ids
            lp_pos, lp_val, lp_ids = lp[0], lp[1].tolist(), lp[2].tolist()
        done = []
        for j, (slot, task) in enumerate(rec["rows"]):
            td = self.state_slot[slot]
            if td["task"] is not task or RequestStatus.is_finished(task.request_status):
                continue
            if td["beam"] is not None:                      # a beam row: its group is handled below, as a whole
                continue
            entry = None
            if lp is not None and j in lp_pos:
                v, i, k = lp_val[lp_pos[j]], lp_ids[lp_pos[j]], task.top_logprobs
                entry = {"logprob": v[0], "top_logprobs": list(zip(i[:k], v[1:1 + k]))}
            self._handle_forward_one_decode_phase(td, int(host_ids[j]), rec["raw"].get(j), entry)
            if RequestStatus.is_finished(task.request_status):
                done.append(slot)
        beam = rec.get("beam")
        if beam is not None:
            for group, row in zip(beam["groups"], beam["out"].tolist()):
                self._handle_beam_step(group, row, done)
        self._process_accomplished_tasks(done)

    def _handle_prompt_logprobs(self, plp):
        """Send the prompt positions one forward computed: plp = (entries, lp [R, 1 + k], ids [R, k]) on the host, entries
        (slot, task, first position, first row, rows).  Rows of a request that has ended meanwhile (abort; the slot may hold a new
        request) are dropped."""
        entries, lp, ids = plp
        lp, ids = lp.tolist(), ids.tolist()
        done = []
        for slot, task, pos, r0, n in entries:
            td = self.state_slot[slot]
            if td["task"] is not task or RequestStatus.is_finished(task.request_status):
                continue
            k, prompt = task.prompt_logprobs, td["plp_prompt"]
            vals = [v[0] for v in lp[r0:r0 + n]]
            tops = [list(zip(i[:k], v[1:1 + k])) for i, v in zip(ids[r0:r0 + n], lp[r0:r0 + n])]
            if pos == 1:                                    # position 0 has no logprob
                pos, vals, tops = 0, [None] + vals, [None] + tops
            task.output_queue.put_nowait(("prompt_logprobs", {"start": pos, "token_ids": prompt[pos:pos + len(vals)],
                                                              "logprobs": vals, "top_logprobs": tops}))
            td["plp_sent"] = pos + len(vals)
            if td["state_category"] == StateCategory.FORWARD_ONE_SUSPENDED and td["plp_sent"] >= len(prompt):
                task.request_status = RequestStatus.FINISHED_LENGTH_CAPPED
                done.append(slot)
        self._process_accomplished_tasks(done)

    def _handle_embeddings(self, entries, sums, lasts, counts):
        """Finish the embeddings whose last chunk one step ran: entries (slot, task, tokens fed); sums / lasts / counts: host copies
        of the accumulator tables' rows of those slots.  A request that has ended meanwhile (abort) is dropped."""
        done = []
        for slot, task, fed in entries:
            td = self.state_slot[slot]
            if td["task"] is not task or RequestStatus.is_finished(task.request_status):
                continue
            count = int(counts[slot])
            vec = finish_embedding(sums[slot].numpy(), lasts[slot].numpy(), count, task.embed, task.embed_normalize)
            task.output_queue.put_nowait(("embedding", {"embedding": vec, "pooled_tokens": count, "prompt_tokens": fed}))
            task.request_status = RequestStatus.FINISHED_LENGTH_CAPPED
            done.append(slot)
        self._process_accomplished_tasks(done)

    def _download_embeddings(self, entries):
        """The record of the embeddings that fed their last token in this step: their slots' accumulator rows copied to pinned host
        memory behind an event.  Two sets of host tables, used in turn: with run-ahead the previous set is read after this step's
        forwards have been enqueued."""
        self._emb_downloads += 1
        if self.device.type != "cuda":
            host = tuple(t.clone() for t in self._emb)
            return {"rows": [], "ids": None, "event": None, "raw": {}, "status": False, "emb": (entries, *host)}
        if self._emb_host is None:
            self._emb_host = [tuple(torch.zeros(t.shape, dtype=t.dtype).pin_memory() for t in self._emb) for _ in range(2)]
        host = self._emb_host[self._emb_downloads & 1]
        for slot, _, _ in entries:
            for h, d in zip(host, self._emb):
                h[slot].copy_(d[slot], non_blocking=True)
        event = torch.cuda.Event()
        event.record()
        return {"rows": [], "ids": None, "event": event, "raw": {}, "status": False, "emb": (entries, *host)}

    def _prompt_rows(self, asks, T: int):
        """Flattened rows b*T + t and their targets (the next prompt token) for the asking batch rows `asks` = [(b, slot)] of a
        forward of T tokens per sequence; advances each slot's prompt cursor.  Returns (rows, targets, entries)."""
        rows, targets, entries = [], [], []
        for b, s in asks:
            td = self.state_slot[s]
            nxt, prompt = td["plp_next"], td["plp_prompt"]
            entries.append((s, td["task"], nxt + 1, len(rows), T))
            rows.extend(range(b * T, b * T + T))
            targets.extend(prompt[nxt + 1:nxt + 1 + T])
            td["plp_next"] = nxt + T
        return rows, targets, entries

    def _upload_int32(self, *lists):
        """One host->device copy of int32 lists (pinned and non-blocking on a GPU: no synchronisation); returns device views."""
        flat = [v for lst in lists for v in lst]
        cuda = self.device.type == "cuda"
        host = torch.tensor(flat, dtype=torch.int32)
        if cuda:
            host = host.pin_memory()
        dev = host.to(self.device, non_blocking=True)
        out, o = [], 0
        for lst in lists:
            out.append(dev[o:o + len(lst)])
            o += len(lst)
        return out

    def _download_plp(self, entries, lp, ids):
        """The prompt-logprob part of a record: device results copied into pinned host memory behind the record's event."""
        if self.device.type != "cuda":
            return (entries, lp, ids)
        hv = torch.empty(lp.shape, dtype=lp.dtype, pin_memory=True)
        hi = torch.empty(ids.shape, dtype=ids.dtype, pin_memory=True)
        hv.copy_(lp, non_blocking=True)
        hi.copy_(ids, non_blocking=True)
        return (entries, hv, hi)

    def _acquire_guides(self, task: Task) -> bool:
        """References on the guides of `task` and of the choices that ride with it, taken at admission (a choice's guide must not be
        dropped before the fork); builds a guide that is new.  On failure -- no room in the pool, a pattern the vocabulary cannot
        realise -- nothing is held, `task` ends aborted with the reason in ``error`` (and an ("error", reason) message), and False
        is returned: its siblings are ended by the caller."""
        group = [t for t in [task] + task.siblings if t.guide is not None]
        if not group:
            return True
        taken = []
        try:
            for t in group:
                taken.append((t, self._pool_for(t.guide).acquire(t.guide, t.stop_tokens)))
        except GuideError as exc:
            for t, (key, _) in taken:
                self._pool_for(t.guide).release(key)
            for t in [task] + task.siblings:
                t.error = f"guided decoding: {exc}"
            task.request_status = RequestStatus.FINISHED_ABORTED
            task.output_queue.put_nowait(("error", task.error))
            task.output_queue.put_nowait(("task_completed", task))
            return False
        for t, ref in taken:
            self._guide_refs[id(t)] = ref
        return True

    def _pool_for(self, guide):
        """The pool of this kind of guide (a StackDFA goes to the grammar pool), allocated on first use."""
        grammar = isinstance(guide, StackDFA)
        pool = self._grammars if grammar else self._guides
        if pool is None:
            pool = (GrammarPool if grammar else GuidePool)(self.grammar_pool_rows if grammar else self.guide_pool_rows, self.real_state_size,
                                                           self.model_config.vocab_size, self.device, getattr(self.tokenizer, "idx2token", None))
            if grammar:
                self._grammars = pool
            else:
                self._guides = pool
        return pool

    def _release_guide(self, task: Task) -> None:
        ref = self._guide_refs.pop(id(task), None)
        if ref is not None:
            self._pool_for(task.guide).release(ref[0])

    def _process_accomplished_tasks(self, slots):
        for s in slots:
            t = self.state_slot[s]["task"]
            self._release_guide(t)
            t.output_queue.put_nowait(("task_completed", t))
            self.state_slot[s] = _empty_slot()

    def _fill_task_pool(self):
        prefills = 0
        for slot in range(self.max_batch_size):
            if prefills >= self.max_prefill_count:
                break
            td = self.state_slot[slot]
            if td["state_category"] != StateCategory.EMPTY:
                prefills += td["state_category"] == StateCategory.FORWARD_SEQ
                continue
            prefills += 1
            task = self._next_task()
            if task is None:
                break
            if task.siblings:
                if not self._admit_group(task, slot):
                    break
                continue
            self._install(task, slot)
            if task.error is not None:                 # refused at admission (its guide): the next request is looked at in this step
                prefills -= 1

    def _next_task(self) -> Optional[Task]:
        """The held group (nothing behind it is admitted first: FIFO), else the next task of the queue; None when there is none.  A
        group of more choices than this worker has slots can never fit (the engine refuses such groups): it ends, aborted."""
        if self._held is not None:
            task, self._held = self._held, None
            return task
        while True:
            try:
                task: Task = self.task_queue.get_nowait()
            except queue.Empty:
                return None
            if task.beam_width and not task.siblings:
                self._make_beam_members(task)
            if 1 + len(task.siblings) <= self.max_batch_size:
                return task
            for t in [task] + task.siblings:
                t.request_status = RequestStatus.FINISHED_ABORTED
                t.output_queue.put_nowait(("task_completed", t))

    def _make_beam_members(self, task: Task) -> None:
        """A beam-search request of width W rides the parallel-choices path: W - 1 internal tasks (no client: _NullSink) are its
        siblings until it ends, so admission, the single prefill, the prefix cache and the fork are those of n = W choices."""
        task.beam_prompt_tokens = len(task.prefill_tokens)   # the tokens fed: behind a prefix-cache hit, the uncached remainder
        members = []
        for j in range(1, task.beam_width):
            t = Task(output_queue=_NullSink(), task_event_queue=queue.Queue(), prompt_str="", prefill_tokens=list(task.prefill_tokens),
                     state=None, task_id=f"{task.task_id}:beam{j}", temperature=0.0, presence_penalty=0.0, frequency_penalty=0.0,
                     penalty_decay=1.0, max_tokens=task.max_tokens, stop_tokens=list(task.stop_tokens), choice_index=j)
            t.beam_leader = task
            members.append(t)
        task.siblings = members

    def _admit_group(self, task: Task, slot: int) -> bool:
        """Parallel choices: choice 0 into `slot` (every slot before it is taken), choices 1..n-1 into the next free slots, suspended
        until the fork.  Only when n slots are free at once; otherwise the group is held (returns False).  One prefill."""
        n = 1 + len(task.siblings)
        free = [s for s in range(slot, self.max_batch_size) if self.state_slot[s]["state_category"] == StateCategory.EMPTY]
        if len(free) < n:
            self._held = task
            return False
        self._install(task, slot)
        td = self.state_slot[slot]
        if td["task"] is not task:                     # ended at admission (an unreachable prefix state): so do its siblings
            for t in task.siblings:
                t.request_status = RequestStatus.FINISHED_ABORTED
                t.output_queue.put_nowait(("task_completed", t))
            return True
        td["siblings"] = list(zip(free[1:n], task.siblings))
        for s, t in td["siblings"]:
            sd = _empty_slot()
            sd.update(task=t, is_prefilling=True, state_category=StateCategory.FORWARD_ONE_SUSPENDED)
            self.state_slot[s] = sd
        self._groups.append((slot, task))
        return True

    def _live_siblings(self, td) -> List[Tuple[int, Task]]:
        return [(s, t) for s, t in td["siblings"] or ()
                if self.state_slot[s]["task"] is t and not RequestStatus.is_finished(t.request_status)]

    def _orphan_on_abort(self, td) -> bool:
        """Choice 0 of a group that has not forked has aborted: when choices are still live its slot prefills on for them (orphan)
        -- the choice itself ends now, and the group's prefix state is not exported.  Returns True for an orphan."""
        if td["orphan"]:
            return True
        if not self._live_siblings(td):
            return False
        t: Task = td["task"]
        t.request_status = RequestStatus.FINISHED_ABORTED
        t.output_queue.put_nowait(("task_completed", t))
        self._release_guide(t)
        td["orphan"] = td["prefill_cached"] = True
        return True

    def _run_forks(self):
        """Groups whose choice-0 slot turned FORWARD_ONE_DECODE in this step (its state holds every prompt token but the last): ONE
        ops.fork_states launch copies each state into the live siblings' slots, behind the forward that produced it and before the
        forward that reads them (stream order, no host synchronisation).  Then the siblings' tables, and every live choice feeds
        the last prompt token as its first decode row.  An orphan's slot is freed; a group whose choices all ended is dropped."""
        forks, keep = [], []
        for p, task in self._groups:
            td = self.state_slot[p]
            if td["task"] is not task:
                continue
            live = self._live_siblings(td)
            if td["orphan"] and not live:              # every choice has aborted: the prefill stops
                self.state_slot[p] = _empty_slot()
                continue
            if td["state_category"] != StateCategory.FORWARD_ONE_DECODE:
                keep.append((p, task))
                continue
            td["siblings"] = None
            forks.append((p, td, live))
        self._groups = keep
        if not any(live for _, _, live in forks):
            return
        assert all(s < self.real_state_size - 1 for _, _, live in forks for s, _ in live)      # never the parking slot
        ops.fork_states(self.batch_state, [(p, [s for s, _ in live]) for p, _, live in forks if live])
        for p, td, live in forks:
            for s, t in live:
                self._write_request_tables(t, s)
                t.prefill_tokens = []
                self.state_slot[s].update(state_category=StateCategory.FORWARD_ONE_DECODE, is_prefilling=False,
                                          next_input_token=td["next_input_token"], prefilled_tokens=list(td["prefilled_tokens"]))
            if td["orphan"]:
                self.state_slot[p] = _empty_slot()
            elif td["task"].beam_width:
                self._start_beam(p, td, live)

    # ------------------------------------------------------------------ beam search
    @staticmethod
    def _is_beam_task(task: Task) -> bool:
        return task.beam_width > 0 or getattr(task, "beam_leader", None) is not None

    def _start_beam(self, p: int, td, live) -> None:
        """The group has forked: position 0 is the leader's slot, positions 1.. the members' slots (ascending).  Position 0 starts
        at score +0, the others at -inf (stream-ordered fills), so the first step chooses among position 0's candidates only."""
        task: Task = td["task"]
        slots, tasks = [p] + [s for s, _ in live], [task] + [t for _, t in live]
        assert len(slots) == task.beam_width
        group = {"task": task, "slots": slots, "tasks": tasks, "W": task.beam_width, "stops": sorted(set(task.stop_tokens)),
                 "parents": [], "ids": [], "hyps": [], "done": False}
        group["K"] = group["W"] + len(group["stops"])
        for pos, s in enumerate(slots):
            self.state_slot[s]["beam"] = (group, pos)
            self.beam_scores[s] = 0.0 if pos == 0 else float("-inf")
        self._beam_live += 1

    def _abort_beam_members(self, td) -> None:
        """The leader of a beam-search request has aborted, before or after the fork: its members end with it (their slots follow
        the leader's in the slot loop of step(), which releases them)."""
        members = [t for _, t in td["siblings"] or ()]
        if td["beam"] is not None:
            td["beam"][0]["done"] = True
            members = td["beam"][0]["tasks"][1:]
            self._beam_live -= 1
        for t in members:
            t.request_status = RequestStatus.FINISHED_ABORTED
        td["task"].siblings = []

    def _beam_step_tables(self, groups, decode_slots):
        """(desc [G, BEAM_DESC_WORDS], the groups' decode rows [R], dst slots [G, 8]) on the device and (first row, W, K) per group, for
        the beam groups of a step; uploaded once per batch composition (pinned, non-blocking) and cached like _slot_tensor."""
        where = {s: j for j, s in enumerate(decode_slots)}
        desc, rows, dst, spans = [], [], [], []
        for g in groups:
            W, out_rows = g["W"], [where[s] for s in g["slots"]]
            desc.append(ops.beam_desc(W, g["stops"], list(range(len(rows), len(rows) + W)), out_rows, g["slots"]))
            spans.append((len(rows), W, g["K"]))
            rows.extend(out_rows)
            dst.append(list(g["slots"]) + [-1] * (ops.BEAM_MAX_W - W))
        key = tuple(v for d in desc for v in d)
        hit = self._beam_tables.get(key)
        if hit is None:
            if len(self._beam_tables) >= 16:
                self._beam_tables.pop(next(iter(self._beam_tables)))
            d, r, t = self._upload_int32([v for x in desc for v in x], rows, [v for x in dst for v in x])
            hit = self._beam_tables[key] = (d.view(len(groups), ops.BEAM_DESC_WORDS), r, t.view(len(groups), ops.BEAM_MAX_W))
        return hit + (spans,)

    def _download_beam(self, groups, spans, bout, bv, bi):
        """The beam part of a record: the step's output records (and, with beam_trace, its candidate tables) copied into pinned host
        memory behind the record's event; two sets used in turn, like the ids."""
        part = {"groups": groups, "spans": spans, "out": bout, "lp": None, "ids": None}
        trace = self.beam_trace
        if self.device.type != "cuda":
            if trace:
                part["lp"], part["ids"] = bv[:, 1:].clone(), bi.clone()
            return part
        if self._beam_host is None:
            n, k = self.real_state_size, ops.TOP_LOGPROBS_MAX
            self._beam_host = [(torch.empty((n * ops.BEAM_OUT_WORDS,), dtype=torch.int32).pin_memory(),
                                torch.empty((n * (k + 1),), dtype=torch.float32).pin_memory(),
                                torch.empty((n * k,), dtype=torch.int32).pin_memory()) for _ in range(2)]
        ho, hv, hi = self._beam_host[self._launches & 1]
        part["out"] = ho[:bout.numel()].view(bout.shape).copy_(bout, non_blocking=True)
        if trace:
            part["lp"] = hv[:bv.numel()].view(bv.shape).copy_(bv, non_blocking=True)[:, 1:]
            part["ids"] = hi[:bi.numel()].view(bi.shape).copy_(bi, non_blocking=True)
        return part

    def _beam_path(self, group, t: int, p: int) -> List[int]:
        """The tokens of the beam in position p after step t (t = 0: none), by backtracking the trellis."""
        toks = []
        for i in range(t - 1, -1, -1):
            toks.append(group["ids"][i][p])
            p = group["parents"][i][p]
        return toks[::-1]

    def _handle_beam_step(self, group, row: List[int], done: List[int]) -> None:
        """Host half of one beam step, one forward behind like every row: extends the trellis, collects the hypotheses the step
        finished, and ends the request after the first step with at least W finished hypotheses or after step max_tokens (every
        live beam with a finite score then ends "length")."""
        task: Task = group["task"]
        if group["done"] or RequestStatus.is_finished(task.request_status):
            return
        def f32(bits: int) -> float:              # the binary32 value a record carries as an int32 word
            return struct.unpack("<f", struct.pack("<i", bits))[0]

        W = group["W"]
        group["parents"].append(row[0:W])
        group["ids"].append(row[24:24 + W])
        t = len(group["ids"])
        for j in range(row[40]):
            group["hyps"].append({"tokens": self._beam_path(group, t - 1, row[41 + j]), "cum": f32(row[57 + j]), "reason": "stop",
                                  "step": t, "order": j})
        if t >= task.max_tokens:
            for p in range(W):
                score = f32(row[32 + p])
                if row[p] >= 0 and math.isfinite(score):
                    group["hyps"].append({"tokens": self._beam_path(group, t, p), "cum": score, "reason": "length", "step": t,
                                          "order": W + row[8 + p]})
        elif len(group["hyps"]) < W:
            return
        self._finish_beam(group, done)

    def _finish_beam(self, group, done: List[int]) -> None:
        """Ranks the hypotheses (cum / max(T, 1) ** length_penalty in binary64; ties: finished earlier, then lower rank), sends the
        one ("beams", ...) message and releases the W slots."""
        task: Task = group["task"]
        lam = task.length_penalty
        for h in group["hyps"]:
            h["score"] = h["cum"] / (float(max(len(h["tokens"]), 1)) ** lam)
        ranked = sorted(group["hyps"], key=lambda h: (-h["score"], h["step"], h["order"]))[:task.beam_n_best]
        out = []
        for h in ranked:
            try:
                text = self.tokenizer.decode(h["tokens"], utf8_errors="ignore")
            except KeyError:             # an id the vocabulary file does not define (the model's vocab is padded)
                text = ""
            out.append({"token_ids": list(h["tokens"]), "text": text, "cumulative_logprob": h["cum"], "score": h["score"],
                        "finish_reason": h["reason"]})
        if out:
            task.generated_tokens, task.decoded_texts = list(out[0]["token_ids"]), [out[0]["text"]]
        stopped = bool(out) and out[0]["finish_reason"] == "stop"
        task.request_status = RequestStatus.FINISHED_STOPPED if stopped else RequestStatus.FINISHED_LENGTH_CAPPED
        task.output_queue.put_nowait(("beams", {"hypotheses": out, "prompt_tokens": getattr(task, "beam_prompt_tokens", 0)}))
        group["done"] = True
        self._beam_live -= 1
        for t in group["tasks"][1:]:
            t.request_status = task.request_status
        task.siblings = []
        done.extend(group["slots"])

    def _install(self, task: Task, slot: int):
        s0, s1, s2 = self.batch_state
        if task.state is None:
            s0[:, :, slot].zero_(), s1[:, slot].zero_(), s2[slot].zero_()
        elif hasattr(task.state, "install_into"):   # prefix-cache hit out of an HbmStateArena: row -> slot, one copy, unpin
            task.state.install_into(self.batch_state, slot)
            task.state.release()
        elif isinstance(task.state, dict) and "__remote_row__" in task.state:
            # process mode: the address of a row in a worker's arena -- this worker's own (one local copy) or another worker's,
            # read through its IPC handle (remote_arena.PeerArenas); the engine learns when the copy has COMPLETED
            wid, row = task.state["__remote_row__"]
            if self.peer_arenas is None:
                raise RuntimeError("a remote arena row arrived at a worker without peer arenas")
            try:
                self.peer_arenas.install(wid, int(row), self.batch_state, slot)
            except Exception as exc:              # noqa: BLE001 -- the owner of the row has ended (its IPC handle cannot be opened,
                # or was never published): that is the end of THIS request -- it holds only the tokens behind the lost prefix --
                # not of this worker and the requests it serves (round-3 advisor finding: the failure used to be fatal for the
                # stealer, one dead worker cascading through the survivors)
                import sys

                print(f"{self.worker_id}: prefix state ({wid}, {row}) is unreachable ({type(exc).__name__}: {exc}); request aborted", file=sys.stderr)
                self.task_queue.installed(task.task_id, wid != self.worker_id)
                task.request_status = RequestStatus.FINISHED_ABORTED
                task.output_queue.put_nowait(("task_completed", task))
                return
            peer = wid != self.worker_id
            if peer and s1.device.type == "cuda":
                ev = torch.cuda.Event()
                ev.record()
                self._pending_installs.append((ev, task.task_id))
            else:                                    # own row: later writers of the row queue behind this copy on this stream
                self.task_queue.installed(task.task_id, peer)
        else:                                    # prefix-cache hit: [L,2,1,C], [L,1,H,64,64], [1]
            s0[:, :, [slot], :] = task.state[0].to(s0.device, non_blocking=True)
            s1[:, [slot], :, :] = task.state[1].to(s1.device, non_blocking=True)
            s2[[slot]] = task.state[2].to(s2.device, non_blocking=True)
        if not self._acquire_guides(task):
            return
        self._write_request_tables(task, slot)
        plp_prompt = list(task.prefill_tokens) if task.prompt_logprobs is not None else None
        if plp_prompt is not None and len(plp_prompt) == 1:      # its one position has no logprob: sent at once
            task.output_queue.put_nowait(("prompt_logprobs", {"start": 0, "token_ids": list(plp_prompt), "logprobs": [None],
                                                              "top_logprobs": [None]}))
            if self._scoring_only(task):
                task.request_status = RequestStatus.FINISHED_LENGTH_CAPPED
                task.output_queue.put_nowait(("task_completed", task))
                return
        first = task.prefill_tokens.pop(0)
        if task.embed is not None:                      # chunks only (every token is fed, the last one too): never a single-token row
            self._reset_embedding(slot)
            cat, prefilling = StateCategory.FORWARD_SEQ, True
        elif len(task.prefill_tokens) == 0:
            cat, prefilling = StateCategory.FORWARD_ONE_DECODE, False
        elif len(task.prefill_tokens) - max(task.cache_prefill_padding - 1, 0) < self.min_forward_seq_len:
            cat, prefilling = StateCategory.FORWARD_ONE_PREFILL, True
        else:
            cat, prefilling = StateCategory.FORWARD_SEQ, True
        td = _empty_slot()
        td.update(task=task, is_prefilling=prefilling, next_input_token=first, state_category=cat, plp_prompt=plp_prompt,
                  plp_sent=1 if plp_prompt is not None and len(plp_prompt) == 1 else 0)
        self.state_slot[slot] = td

    def _reset_embedding(self, slot: int):
        """The slot's embedding accumulators, zeroed at admission (allocated on the first embedding request).  Stream-ordered writes:
        the copies of the slot's previous embedding to the host were enqueued before them."""
        if self._emb is None:
            n, C, dev = self.real_state_size, int(self.batch_state[0].shape[3]), self.device
            self._emb = (torch.zeros((n, C), dtype=torch.float32, device=dev), torch.zeros((n, C), dtype=torch.float16, device=dev),
                         torch.zeros((n,), dtype=torch.int32, device=dev))
        for t in self._emb:
            t[slot].zero_()

    def _write_request_tables(self, task: Task, slot: int):
        """The slot's penalty, sampling, seed and bias tables for `task` (at admission; a sibling choice's at the fork)."""
        self.occurrence[slot].zero_()
        self.alpha_presence_vector[slot].zero_()
        if getattr(self, "_pen_lists", None) is not None:
            self._pen_lists.reset(slot)
        beam = self._is_beam_task(task)          # the search reads the raw output: zero penalties, no draw, no seed
        self.temperature_tensor[slot, 0] = task.temperature if task.temperature > 0 else 1.0
        self.top_p_tensor[slot, 0] = task.top_p
        self.top_k_tensor[slot, 0] = task.top_k
        self.frequency_penalty_tensor[slot, 0] = 0.0 if beam else task.frequency_penalty
        self.penalty_decay_tensor[slot, 0] = 1.0 if beam else task.penalty_decay
        self.presence_penalty_tensor[slot, 0] = 0.0 if beam else task.presence_penalty
        self._greedy[slot] = beam or is_greedy_row(task.temperature, task.top_p, task.top_k)
        # stream-ordered writes: a run-ahead row of the slot's previous request still in flight reads (and advances) the old values
        seeded = task.seed is not None and not beam
        if seeded or self._seeded[slot]:
            self.seeds[slot] = ops.seed_int64(task.seed) if seeded else 0
            self.seeded[slot] = 1 + task.choice_index if seeded else 0     # Philox stream of the choice
            self.counters[slot] = 0
            self._seeded[slot] = seeded
        n_bias = len(task.logit_bias)
        if n_bias or self._bias_n[slot]:
            if n_bias:
                self.bias_ids[slot, :n_bias] = torch.tensor(list(task.logit_bias.keys()), dtype=torch.int32)
                self.bias_values[slot, :n_bias] = torch.tensor(list(task.logit_bias.values()), dtype=torch.float32)
            self.bias_counts[slot] = n_bias
            self._bias_n[slot] = n_bias
        ref = self._guide_refs.get(id(task))
        grammar = ref is not None and isinstance(task.guide, StackDFA)
        if (ref is not None and not grammar) or self._guided[slot]:
            self._guides.state[slot] = ref[1] if ref is not None and not grammar else -1      # the guide's start row
            self._guided[slot] = ref is not None and not grammar
        if grammar or self._grammared[slot]:               # start row and empty stack (-1: the slot's previous request had a grammar):
            self._grammar_resets[slot] = ref[1] if grammar else -1      # one launch for all of them, in front of the next forward
            self._grammared[slot] = grammar

    def _organize_batch(self):
        """Slot ids per category, in slot order (the reference returns contiguous ranges after
        swapping; here the lists ARE the addressing)."""
        by_cat: Dict[StateCategory, List[int]] = {c: [] for c in StateCategory}
        for slot in range(self.max_batch_size):
            by_cat[self.state_slot[slot]["state_category"]].append(slot)
        return by_cat

    # ------------------------------------------------------------------ device dispatch
    def _slot_tensor(self, slots: List[int]) -> torch.Tensor:
        """Device copy of a list of slot / row ids, cached: torch.tensor(list, device=...) is a pageable host-to-device copy, i.e.
        the host blocks until everything already enqueued on the stream has run -- once per iteration that turned the run-ahead loop into
        a lock-step one (the GPU idled ~200 us per 7-ms iteration while the host enqueued the next).  The decode slot list is the same
        from one iteration to the next until a request arrives or leaves; the tensors are never written."""
        key = tuple(slots)
        t = self._slot_cache.get(key)
        if t is None:
            if len(self._slot_cache) >= 16:
                self._slot_cache.pop(next(iter(self._slot_cache)))
            t = self._slot_cache[key] = torch.tensor(slots, dtype=torch.int32, device=self.device)
        return t

    def _run_forward_one(self, decode_slots: List[int], prefill_slots: List[int]):
        """Enqueue one forward + sampling for these slots; returns the record `_handle_results` consumes."""
        slots = decode_slots + prefill_slots
        if not slots:
            return None
        if self._grammar_resets:                           # the slots admitted or forked since the last forward (a group of choices: all
            pending, self._grammar_resets = self._grammar_resets, {}     # at once); in stream order behind the last step's advance
            ops.grammar_reset(torch.tensor(list(pending), dtype=torch.int32).to(self.device),
                              torch.tensor(list(pending.values()), dtype=torch.int32).to(self.device),
                              self._grammars.state, self._grammars.stack)
        idx = self._slot_tensor(slots)
        nd = len(decode_slots)
        # every small host->device tensor is created BEFORE the forward is enqueued: a pageable H2D copy is
        # synchronous and would otherwise stall the host behind the whole decode step
        sampled = [j for j, s in enumerate(decode_slots) if not self._greedy[s]]
        rows = u = None
        if sampled:
            rows = self._slot_tensor(sampled)
            u = torch.rand((len(sampled),), device=self.device, dtype=torch.float32)
            # seeded rows replace their uniform with their own Philox draw (the unseeded rows' draws stay those of the global
            # generator, consumed exactly as before)
            seeded_rows = [k for k, j in enumerate(sampled) if self._seeded[decode_slots[j]]]
            if seeded_rows:
                ops.seeded_uniform(rows, idx, self.seeds, self.seeded, self.counters, u)
        lp_rows = [j for j, s in enumerate(decode_slots) if self.state_slot[s]["task"].logprobs]
        g_rows = [j for j, s in enumerate(decode_slots) if self._guided[s]]
        g_idx = self._slot_tensor(g_rows) if g_rows else None
        s_rows = [j for j, s in enumerate(decode_slots) if self._grammared[s]]
        s_idx = self._slot_tensor(s_rows) if s_rows else None
        # single-token prefill rows that ask for prompt logprobs: their row list and targets, uploaded before the forward
        p_asks = [(nd + j, s) for j, s in enumerate(prefill_slots) if self.state_slot[s]["plp_prompt"] is not None]
        if p_asks:
            p_k = max(self.state_slot[s]["task"].prompt_logprobs for _, s in p_asks)
            p_rows, p_targets, p_entries = self._prompt_rows(p_asks, 1)
            p_rows_dev, p_targets_dev = self._upload_int32(p_rows, p_targets)
        if lp_rows:
            lp_idx = self._slot_tensor(lp_rows)
            lp_k = max(self.state_slot[decode_slots[j]]["task"].top_logprobs for j in lp_rows)
        # beam groups of the step (all W slots of a forked group decode together until it ends): their tables, before the forward
        b_groups = ([td["beam"][0] for td in (self.state_slot[s] for s in decode_slots) if td["beam"] is not None and td["beam"][1] == 0]
                    if self._beam_live else [])
        if b_groups:
            b_desc, b_rows, b_dst, b_spans = self._beam_step_tables(b_groups, decode_slots)
        tokens = []
        for j, s in enumerate(slots):
            td = self.state_slot[s]
            tokens.append(-1 if (j < nd and td["feedback"]) else td["next_input_token"])    # -1: last_ids[slot]
            if j < nd:
                td["feedback"] = True
        if self.use_graph:
            out = self._graph_for(len(slots)).run(tokens, slots)
        else:
            tok = torch.tensor(tokens, dtype=torch.long, device=self.device).view(-1, 1)
            tok = torch.where(tok < 0, self.last_ids[idx.long()].long().view(-1, 1), tok)
            out = self.model.forward_slots(tok, self.batch_state, idx)
        self._launches += 1
        plp = None
        if p_asks:
            # out[nd:] are the prefill rows: the penalties, bias and forbidden tokens below edit out[:nd] only, and this launch runs
            # before the next forward can overwrite a graph's static output buffer
            pv, pi = ops.token_logprobs(out, p_k, targets=p_targets_dev, rows=p_rows_dev)
            plp = self._download_plp(p_entries, pv, pi)
        if b_groups:
            # the K = W + S most likely ids of each beam row and their log-probabilities, of the raw output: before any edit below
            bv, bi = ops.token_logprobs(out, max(g["K"] for g in b_groups), rows=b_rows)
        if nd == 0:
            if plp is None:
                return None
            event = None
            if self.device.type == "cuda":
                event = torch.cuda.Event()
                event.record()
            return {"rows": [], "ids": None, "event": event, "raw": {}, "status": False, "plp": plp}
        logits = out[:nd]
        # logprobs are those of the raw model output: the rows that ask are copied before the forbidden tokens and the penalty
        # kernel edit `logits` in place (the graph's output buffer is static)
        snap = logits.index_select(0, lp_idx) if lp_rows else None
        raw = {}
        for j, s in enumerate(decode_slots):
            t: Task = self.state_slot[s]["task"]
            if t.return_logits:
                raw[j] = logits[j].clone()
            for tok_id in t.forbidden_tokens:
                logits[j, tok_id] -= 1e10
        didx = idx[:nd]
        if any(self._bias_n[s] for s in decode_slots):     # after the forbidden tokens, before the penalties and every draw
            ops.apply_logit_bias(logits, didx, self.bias_counts, self.bias_ids, self.bias_values)
        if g_rows:                                         # after the bias (a bias cannot re-admit a token), before the penalties
            ops.guide_apply(logits, g_idx, didx, self._guides.state, self._guides.allow)
        if s_rows:                                         # the rows under a grammar, in the same place
            G = self._grammars
            ops.grammar_apply(logits, s_idx, didx, G.state, G.stack, G.next, G.meta, G.allow, G.maybe, G.tok_off, G.tok_bytes)
        # penalties for every decode row + arg-max, one kernel; occurrence is decayed in place
        status_out = None
        if self._commit_kernel is not None and self.device.type == "cuda":
            buf = torch.empty((nd + 1,), dtype=torch.int32, device=self.device)     # the ids, and the launch-status word behind them
            ids, status_out = buf[:nd], buf[nd:]
            self._penalize_argmax(logits, self.occurrence, self.alpha_presence_vector, self.penalty_decay_tensor.view(-1),
                                  self.frequency_penalty_tensor.view(-1), didx, out=ids, **({"lists": self._pen_lists} if self._pen_lists is not None else {}))
        else:
            ids = self._penalize_argmax(logits, self.occurrence, self.alpha_presence_vector, self.penalty_decay_tensor.view(-1),
                                        self.frequency_penalty_tensor.view(-1), didx)
        if sampled:
            if self._sample_topp is not None and logits.shape[1] <= 65536:
                # sort-free top-p / top-k / temperature kernel, one workgroup per sampled row
                self._sample_topp(logits, rows, self.temperature_tensor.view(-1), self.top_p_tensor.view(-1),
                                  self.top_k_tensor.view(-1), u, ids, didx)
            else:
                lrows = rows.long()
                srows = didx.long()[lrows]
                drawn = sample_logits_rwkv_pip_compatible(logits[lrows], self.temperature_tensor[srows],
                                                          self.top_p_tensor[srows], self.top_k_tensor[srows])
                if seeded_rows:                             # every row still drew above: the generator advances as without seeds
                    k = torch.tensor(seeded_rows, dtype=torch.long, device=self.device)
                    drawn[k] = sample_inverse_cdf(logits[lrows[k]], self.temperature_tensor[srows[k]], self.top_p_tensor[srows[k]],
                                                  self.top_k_tensor[srows[k]], u[k])
                ids[lrows] = drawn.to(torch.int32)
        if b_groups:
            # the next beams, on the device: their ids replace the beam rows' arg-max ids before the commit feeds them back, and
            # the states the selection moves are copied behind the commit and before the next forward -- no host round trip
            # (filled with -1: a group the kernel refuses writes nothing, and its record then reads as no beams and no hypotheses)
            bout = torch.full((len(b_groups), ops.BEAM_OUT_WORDS), -1, dtype=torch.int32, device=self.device)
            ops.beam_select(bv[:, 1:], bi, b_desc, self.beam_scores, ids, bout)
        self._commit_sampled(ids, didx, status_out)
        if b_groups:
            ops.beam_copy_states(self.batch_state, bout[:, ops.BEAM_OUT_COPY:ops.BEAM_OUT_COPY + ops.BEAM_MAX_W], b_dst)
        if g_rows:                                         # the sampled ids move the guided slots' states, on the device
            ops.guide_advance(g_idx, didx, ids, self._guides.tok_off, self._guides.tok_bytes, self._guides.next, self._guides.state)
        if s_rows:                                         # ... and the grammar slots' states and stacks
            G = self._grammars
            ops.grammar_advance(s_idx, didx, ids, G.tok_off, G.tok_bytes, G.next, G.meta, G.state, G.stack)
        lp = None
        if lp_rows:                                         # the sampled ids are read on the device, in place
            lp_val, lp_ids = ops.token_logprobs(snap, lp_k, targets=ids, target_rows=lp_idx)
            lp = [{j: p for p, j in enumerate(lp_rows)}, lp_val, lp_ids]
        event = None
        if self._ids_host is not None:
            host = self._ids_host[self._launches & 1]
            if status_out is not None:
                host[:nd + 1].copy_(buf, non_blocking=True)
            else:
                host[:nd].copy_(ids, non_blocking=True)
            if lp is not None:                              # double-buffered like the ids: the loop runs one forward ahead
                if self._lp_host is None:
                    n_max, k_max = self.real_state_size, ops.TOP_LOGPROBS_MAX
                    self._lp_host = [(torch.empty((n_max * (k_max + 1),), dtype=torch.float32).pin_memory(),
                                      torch.empty((n_max * k_max,), dtype=torch.int32).pin_memory()) for _ in range(2)]
                hv, hi = self._lp_host[self._launches & 1]
                n_lp = len(lp_rows)
                lp[1] = hv[:lp_val.numel()].view(n_lp, lp_k + 1).copy_(lp_val, non_blocking=True)
                lp[2] = hi[:lp_ids.numel()].view(n_lp, lp_k).copy_(lp_ids, non_blocking=True)
            if b_groups:
                beam = self._download_beam(b_groups, b_spans, bout, bv, bi)
            event = torch.cuda.Event()
            event.record()
            ids = host
        elif b_groups:
            beam = self._download_beam(b_groups, b_spans, bout, bv, bi)
        rec = {"rows": [(s, self.state_slot[s]["task"]) for s in decode_slots], "ids": ids, "event": event, "raw": raw,
               "status": status_out is not None and self._ids_host is not None}
        if b_groups:
            rec["beam"] = beam
        if lp is not None:
            rec["lp"] = lp
        if plp is not None:
            rec["plp"] = plp
        return rec

    def _graph_for(self, n: int):
        """Smallest captured bucket >= n (buckets: powers of two up to the slot count)."""
        from .rwkv7 import SlotDecodeGraph

        b = 1
        while b < n:
            b *= 2
        b = min(b, self.max_batch_size)
        g = self._graphs.get(b)
        if g is None:
            g = self._graphs[b] = SlotDecodeGraph(self.model, self.batch_state, b, parking_slot=self.real_state_size - 1,
                                                  feedback=self.last_ids)
        return g

    def _seq_left(self, s: int) -> int:
        """Tokens the chunk path may still feed for slot s: everything but the last prompt token (a single-token row feeds it) and
        the cache padding -- for an embedding request every token that is left."""
        td = self.state_slot[s]
        t: Task = td["task"]
        if t.embed is not None:
            return 1 + len(t.prefill_tokens)
        return len(t.prefill_tokens) - max(t.cache_prefill_padding - 1, 0)

    def _run_forward_seq(self, seq_slots: List[int]):
        """The chunk forward(s) of a step.  Without an embedding request among the slots: one forward, as ever.  An embedding is fed
        to its very last token by chunks, so what is left of one can be shorter than min_forward_seq_len, the least any other
        sequence brings -- and one forward feeds every sequence the same number of tokens.  Rule: the embedding slots with fewer
        than min_forward_seq_len tokens left run in a forward of their own, behind the others'; nobody's chunk gets shorter than it
        would have been without them."""
        if not any(self.state_slot[s]["task"].embed is not None for s in seq_slots):
            return self._run_chunk(seq_slots, None)
        short = [s for s in seq_slots if self.state_slot[s]["task"].embed is not None and self._seq_left(s) < self.min_forward_seq_len]
        recs, finishing = [], []
        for group in ([s for s in seq_slots if s not in short], short):
            if group:
                rec = self._run_chunk(group, finishing)
                if rec is not None:
                    recs.append(rec)
        if finishing:
            recs.append(self._download_embeddings(finishing))
        return recs or None

    def _run_chunk(self, seq_slots: List[int], finishing):
        """One chunk forward of these slots; finishing collects (slot, task, tokens fed) of the embeddings that fed their last token."""
        lens = [self._seq_left(s) for s in seq_slots]
        n_tok = min(self.max_forward_seq_len_per_forward, *lens)
        assert n_tok > 0
        asks = [(b, s) for b, s in enumerate(seq_slots) if self.state_slot[s]["plp_prompt"] is not None]
        if asks:                                            # (before the cursors below move)
            k = max(self.state_slot[s]["task"].prompt_logprobs for _, s in asks)
            rows, targets, entries = self._prompt_rows(asks, n_tok)
        batch, pools = [], []
        for b, s in enumerate(seq_slots):
            td = self.state_slot[s]
            t: Task = td["task"]
            chunk = [td["next_input_token"]] + t.prefill_tokens[: n_tok - 1]
            td["prefilled_tokens"].extend(chunk)
            t.prefill_tokens = t.prefill_tokens[n_tok - 1:]
            if t.embed is not None:
                # (batch row, first pooled position of the chunk, slot): the leading embed_skip prompt positions are left out
                pools.append((b, min(max(t.embed_skip - td["emb_fed"], 0), n_tok), s))
                td["emb_fed"] += n_tok
                td["next_input_token"] = t.prefill_tokens.pop(0) if t.prefill_tokens else None
                if td["next_input_token"] is None:      # its last token is in this chunk: it waits for the pooled rows, then ends
                    td["state_category"], td["is_prefilling"] = StateCategory.FORWARD_ONE_SUSPENDED, False
                    finishing.append((s, t, td["emb_fed"]))
            else:
                td["next_input_token"] = t.prefill_tokens.pop(0)
            batch.append(chunk)
        kw = {}
        if pools:                                           # (only then: a backend without embeddings never sees the keyword)
            kw["pool_rows"] = (*self._upload_int32(*[list(col) for col in zip(*pools)]), *self._emb)
        if not asks:
            self.model.forward_slots(batch, self.batch_state, self._slot_tensor(seq_slots), **kw)   # logits discarded (:776)
            return None
        # prompt logprobs: the head output of every row of the asking sequences, a block at a time, straight into the logprob
        # kernel (the target of row (b, t) is the prompt token after it); the results reach the host behind an event like the ids
        rows_dev, targets_dev = self._upload_int32(rows, targets)
        lp = torch.empty((len(rows), k + 1), dtype=torch.float32, device=self.device)
        ids = torch.empty((len(rows), k), dtype=torch.int32, device=self.device)

        def sink(r0, block):
            v, i = ops.token_logprobs(block, k, targets=targets_dev[r0:r0 + block.shape[0]])
            lp[r0:r0 + block.shape[0]].copy_(v)
            ids[r0:r0 + block.shape[0]].copy_(i)

        self.model.forward_slots(batch, self.batch_state, self._slot_tensor(seq_slots), logit_rows=rows_dev, row_sink=sink, **kw)
        event = None
        plp = self._download_plp(entries, lp, ids)
        if self.device.type == "cuda":
            event = torch.cuda.Event()
            event.record()
        return {"rows": [], "ids": None, "event": event, "raw": {}, "status": False, "plp": plp}

    # ------------------------------------------------------------------ main loop
    def step(self) -> bool:
        """One loop iteration (chirrup/worker.py:793-884).  Returns False when idle.
        Order: (1) host-only slot bookkeeping that needs no sampled token (aborts, prompt cursors, admission),
        (2) enqueue this iteration's forward(s), (3) handle sampled ids -- those of the PREVIOUS iteration's
        forward when running ahead, else this one's."""
        t0 = time.perf_counter()
        poll_exports = getattr(self.task_queue, "poll_exports", None)
        if poll_exports is not None:                   # process mode: row addresses whose export copies have completed may leave now
            poll_exports()
        if self._pending_installs:                     # copies out of another worker's arena: report those that have completed
            still = []
            for ev, task_id in self._pending_installs:
                if ev.query():
                    self.task_queue.installed(task_id, True)
                else:
                    still.append((ev, task_id))
            self._pending_installs = still
        done = []
        for slot in range(self.max_batch_size):
            td = self.state_slot[slot]
            cat = td["state_category"]
            assert cat != StateCategory.FINISHED
            if cat == StateCategory.EMPTY:
                continue
            if self._is_task_aborted(td) and not (td["siblings"] and not td["task"].beam_width and self._orphan_on_abort(td)):
                td["task"].request_status = RequestStatus.FINISHED_ABORTED
                td["state_category"] = StateCategory.FINISHED
                if td["task"].beam_width:
                    self._abort_beam_members(td)
            elif cat == StateCategory.FORWARD_SEQ:
                self._handle_forward_seq(td, slot)
            elif cat == StateCategory.FORWARD_ONE_PREFILL:
                self._handle_forward_one_prefill_phase(td, slot)
            if RequestStatus.is_finished(td["task"].request_status) and not td["orphan"]:
                done.append(slot)
        self._process_accomplished_tasks(done)
        self._fill_task_pool()
        if self._groups:
            self._run_forks()
        cats = self._organize_batch()
        dec, pre, seq = (cats[c] for c in (StateCategory.FORWARD_ONE_DECODE, StateCategory.FORWARD_ONE_PREFILL,
                                           StateCategory.FORWARD_SEQ))
        if not dec and not pre and not seq:
            if self._inflight is None:
                return False
            rec, self._inflight = self._inflight, None           # drain the pipeline
            self._handle_results(rec)
            return True
        rec = None
        if dec or pre:
            rec = self._run_forward_one(dec, pre)
            self.seq_forward_count_down -= 1
        else:
            self.seq_forward_count_down = 0
        if seq and (self.seq_forward_count_down < 1 or (self.prefill_when_underfilled and 2 * len(dec) < self.max_batch_size)):
            rec_seq = self._run_forward_seq(seq)
            self.seq_forward_count_down = max(1, self.decode_prefill_ratio)
            if rec_seq is not None:                         # (prompt logprobs of the chunk: handled with this step's other results)
                rec = [rec, rec_seq] if rec is not None else rec_seq
        if self.run_ahead:
            rec, self._inflight = self._inflight, rec
        self._handle_results(rec)
        self.iterations += 1
        self.loop_time_recorder.append(time.perf_counter() - t0)
        if (self.iterations & 63) == 1 or self._max_mem_gb is None:      # (memory_stats() walks a dictionary of ~150 counters: 0.12 ms per call)
            self._max_mem_gb = (torch.cuda.max_memory_allocated() / 1024 ** 3) if torch.cuda.is_available() else 0.0
        self._post({"avg_loop_time": sum(self.loop_time_recorder) / len(self.loop_time_recorder),
                    "state_size": self.real_state_size,
                    "state_offset_details": {"decode_slots": dec, "one_prefill_slots": pre, "seq_prefill_slots": seq},
                    "task_details": {"decode_count": len(dec), "one_prefill_count": len(pre), "seq_prefill_count": len(seq)},
                    "max_allocated_memory_GB": self._max_mem_gb},
                   "worker_performance")
        return True

    def start(self):
        """The worker thread's entry point.  A failure anywhere in the loop must not strand the clients: it is
        reported on the worker event queue and on stderr, and every request this worker holds is completed as
        aborted before the thread ends (the reference's loop has no such path: a dead worker thread leaves its
        requests waiting forever)."""
        try:
            if self.batch_state is None:
                self._init_worker()
            while True:
                if self._process_events():
                    break
                if not self.step():
                    time.sleep(0.05)
        except BaseException as exc:             # noqa: BLE001 -- report, release the clients, then re-raise
            import traceback

            traceback.print_exc()
            self._post({"status": "failed", "worker_id": self.worker_id, "error": repr(exc)}, "worker_error")
            self._fail_all_requests()
            if self.on_fatal is not None:
                self.on_fatal(self, exc)         # the engine releases queued requests if no worker is left
            raise
        finally:
            self._cleanup()

    def _fail_all_requests(self):
        held = getattr(self, "_held", None)
        tasks = [td.get("task") for td in list(getattr(self, "state_slot", {}).values())] + ([held] + held.siblings if held else [])
        for t in tasks:
            if t is not None and not RequestStatus.is_finished(t.request_status):
                t.request_status = RequestStatus.FINISHED_ABORTED
                try:
                    t.output_queue.put_nowait(("task_completed", t))
                except Exception:                # noqa: BLE001
                    pass

    def _cleanup(self):
        for name in ("state_slot", "batch_state", "occurrence", "alpha_presence_vector", "model"):
            if hasattr(self, name):
                delattr(self, name)


def model_load_config_for(model_path: str, vocab_path: str, vocab_size: int = 65536) -> ModelLoadConfig:
    return ModelLoadConfig(model_path=model_path, vocab_path=vocab_path, vocab_size=vocab_size, head_size=64)


__all__ = ["Worker", "GuidePool", "GrammarPool", "StateCategory", "min_swaps_to_target_fast", "types"]
