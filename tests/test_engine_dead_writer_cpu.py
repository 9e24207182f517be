"""Process mode: a worker process that dies WHILE IT HOLDS THE WRITE LOCK of the shared result queue (its queue feeder thread is
in the middle of a message when a HIP abort, a kill or os._exit takes the process).  Nobody can write to that queue afterwards, so
the news of the death must not travel through it: the liveness monitor tells the router directly, the worker's requests complete as
aborted, the handle reports the process dead, and neither shutdown() nor the interpreter's exit waits for the wedged queue."""
import asyncio
import os
import subprocess
import sys

from chirrup_amd.core_structure import ModelLoadConfig
from chirrup_amd.engine_core import AsyncEngineCore
from chirrup_amd.worker import Worker
from test_worker_cpu import FakeModel, FakeTok, V, cpu_penalize_argmax

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Tok(FakeTok):
    def encode(self, s):
        return [ord(c) % (V - 1) + 1 for c in s]


class _DiesHoldingTheLock(FakeModel):
    """On its fourth forward: takes the result queue's write lock, as the queue's feeder thread does around every message it
    sends, and ends the process without releasing it.  A worker that streams tokens is inside that lock whenever something kills
    it; taking the lock here (``multiprocessing.Queue`` has no public handle on it, hence ``_wlock``) makes the case happen every
    time -- ending the process "while a large message is on its way" only wedges the queue when the timing falls right."""
    calls, result_q = 0, None

    def forward_slots(self, *a, **k):
        type(self).calls += 1
        if type(self).calls >= 4:
            self.result_q._wlock.acquire()
            os._exit(1)
        return super().forward_slots(*a, **k)


def _factory(**kw):
    _DiesHoldingTheLock.result_q = kw["worker_event_queue"]._q
    return Worker(model=_DiesHoldingTheLock(), tokenizer=_Tok(), penalize_argmax=cpu_penalize_argmax, **kw)


async def _main():
    eng = AsyncEngineCore(worker_factory=_factory, tokenizer=_Tok(), worker_mode="process")
    cfg = ModelLoadConfig(model_path="fake", vocab_path="fake", vocab_size=V, head_size=64)
    await asyncio.wait_for(eng.init(worker_num=1, model_config=cfg, batch_size=3), 120)
    kw = dict(temperature=0.0, frequency_penalty=0.0, presence_penalty=0.0, penalty_decay=1.0, stop_tokens=[], max_tokens=10 ** 6)
    cs = [eng.completion("", prefill_tokens=[1, 2, 3], **kw) for _ in range(4)]             # two running, two queued
    await asyncio.wait_for(asyncio.gather(*[c.get_full_completion() for c in cs]), 30)
    assert all(str(c.task.request_status) == "FINISHED_ABORTED" for c in cs)
    assert not eng.workers[0].is_alive() and eng.workers[0].process.exitcode == 1
    eng.shutdown()


def test_a_worker_that_dies_holding_the_result_queue_lock_releases_its_clients():
    asyncio.run(_main())


def test_the_wedged_queue_does_not_hold_up_the_interpreters_exit():
    """The same in a process of its own, which then has to END: the put that shutdown() leaves in the wedged queue must not be
    waited for at exit."""
    code = ("import sys, asyncio; sys.path[:0] = [%r, %r]; import test_engine_dead_writer_cpu as t; asyncio.run(t._main()); print('done')"
            % (ROOT, os.path.join(ROOT, "tests")))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("done"), out.stderr[-2000:]
