"""Token logprobs without a GPU: the worker's plumbing over the CPU fake model (ops.token_logprobs' torch form), the OpenAI shape of
/v1/chat/completions over the fake-backend engine, the C ABI's argument checks, and the kernel's register report."""
import asyncio
import ctypes
import json
import math
import os
import re
import shutil
import subprocess

import httpx
import pytest
import torch

from chirrup_amd import ops
from chirrup_amd.core_structure import ModelLoadConfig
from chirrup_amd.engine_core import AsyncEngineCore
from chirrup_amd.web_service import ChatCompletionRequest, ChatMessage, chat_prompt, create_app
from test_engine_cpu import _factory, _Tok
from test_worker_cpu import V, expected_stream, make_worker, new_task, run_until_idle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _payloads(task):
    return [p for kind, p in task.output_queue.items if kind == "token_generated"]


def _log_softmax64(raw):
    x = [float(v) for v in raw.float().tolist()]
    m = max(x)
    z = math.log(sum(math.exp(v - m) for v in x))
    return [(v - m) - z for v in x]


def test_ops_token_logprobs_torch_form_definition():
    lg = torch.tensor([[1, 3, 3, 2, 0, 0, 0, 0], [0] * 8], dtype=torch.float16)
    lp, ids = ops.token_logprobs(lg, 3, targets=torch.tensor([2, 9], dtype=torch.int32))
    assert ids.tolist() == [[1, 2, 3], [0, 1, 2]]             # logit descending, ties by id
    want = _log_softmax64(lg[0])
    assert abs(lp[0, 0].item() - want[2]) < 1e-6 and math.isnan(lp[1, 0].item())
    assert all(abs(lp[0, 1 + j].item() - want[i]) < 1e-6 for j, i in enumerate([1, 2, 3]))
    lp, ids = ops.token_logprobs(lg, 0, rows=torch.tensor([1], dtype=torch.int32))
    assert lp.shape == (1, 1) and ids.shape == (1, 0)
    with pytest.raises(Exception):
        ops.token_logprobs(lg, 21)


def test_task_validates_top_logprobs():
    with pytest.raises(ValueError):
        new_task([1, 2], top_logprobs=3)
    with pytest.raises(ValueError):
        new_task([1, 2], logprobs=True, top_logprobs=21)
    new_task([1, 2], logprobs=True, top_logprobs=20)


def test_worker_emits_one_logprob_entry_per_generated_token():
    w, tq, _, _ = make_worker()
    prompt = [5, 9, 2]
    stream = expected_stream(prompt, 8)
    stop = stream[5]
    t_lp = new_task(prompt, max_tokens=8, logprobs=True, top_logprobs=4, return_logits=True, stop_tokens=[stop])
    t_lp0 = new_task(prompt, max_tokens=8, logprobs=True)
    t_plain = new_task(prompt, max_tokens=8, return_logits=True)
    t_bare = new_task(prompt, max_tokens=8)
    for t in (t_lp, t_lp0, t_plain, t_bare):
        tq.put(t)
    run_until_idle(w)
    got = _payloads(t_lp)
    assert [p[0] for p in got] == stream[:stream.index(stop)] == t_lp.generated_tokens     # the stop token: no entry
    for tok, text, raw, lp in got:
        assert set(lp) == {"logprob", "top_logprobs"} and len(lp["top_logprobs"]) == 4
        want = _log_softmax64(raw)
        assert abs(lp["logprob"] - want[tok]) < 1e-5
        assert lp["top_logprobs"][0][0] == tok                 # greedy, no penalties
        assert all(abs(v - want[i]) < 1e-5 for i, v in lp["top_logprobs"])
    assert [p[0] for p in _payloads(t_lp0)] == stream
    assert all(len(p) == 4 and p[2] is None and p[3]["top_logprobs"] == [] for p in _payloads(t_lp0))
    assert all(len(p) == 3 for p in _payloads(t_plain)) and all(len(p) == 2 for p in _payloads(t_bare))


def test_steps_without_logprob_rows_never_call_the_kernel(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("token_logprobs called in a step where no row asked")

    monkeypatch.setattr(ops, "token_logprobs", boom)
    w, tq, _, _ = make_worker()
    t = new_task([1, 2, 3], max_tokens=5, return_logits=True)
    tq.put(t)
    run_until_idle(w)
    assert len(t.generated_tokens) == 5 and w._lp_host is None
    t = new_task([1, 2, 3], max_tokens=5, logprobs=True)
    tq.put(t)
    with pytest.raises(AssertionError, match="no row asked"):
        run_until_idle(w)


class _VocabTok(_Tok):
    """The fake tokenizer with a vocabulary table; ids 40.. are padding (not in the file)."""
    idx2token = {i: (b"\xff" if i == 3 else f"t{i}".encode()) for i in range(40)}


async def _app_client():
    eng = AsyncEngineCore(worker_factory=_factory, tokenizer=_VocabTok())
    cfg = ModelLoadConfig(model_path="fake", vocab_path="fake", vocab_size=V, head_size=64)
    await eng.init(worker_num=1, model_config=cfg, batch_size=4)
    app = create_app(eng, state_cache_size=0)
    return eng, httpx.AsyncClient(transport=httpx.ASGITransport(app=app), base_url="http://t")


def _entry(tok, lp):
    b = _VocabTok.idx2token.get(tok, b"")
    return b.decode("utf-8", errors="backslashreplace"), list(b)


def test_chat_logprobs_non_streamed_and_streamed():
    async def main():
        eng, cl = await _app_client()
        msgs = [{"role": "user", "content": "count the slots"}]
        req = {"model": "rwkv-latest:no-thinking", "messages": msgs, "temperature": 0.0, "top_p": 0.0, "presence_penalty": 0.0,
               "frequency_penalty": 0.0, "penalty_decay": 1.0, "max_tokens": 7}
        prompt, _ = chat_prompt([ChatMessage(**x) for x in msgs], req["model"])
        stream = expected_stream([0] + _Tok().encode(prompt), 7)
        async with cl:
            plain = await cl.post("/v1/chat/completions", json=req)
            assert "logprobs" not in plain.json()["choices"][0] and b"logprobs" not in plain.content
            j = (await cl.post("/v1/chat/completions", json=dict(req, logprobs=True, top_logprobs=3))).json()
            ch = j["choices"][0]
            assert list(ch) == ["index", "finish_reason", "message", "logprobs"] and ch["message"] == plain.json()["choices"][0]["message"]
            content = ch["logprobs"]["content"]
            assert len(content) == 7
            for tok, e in zip(stream, content):
                assert set(e) == {"token", "logprob", "bytes", "top_logprobs"}
                assert (e["token"], e["bytes"]) == _entry(tok, e["logprob"])
                assert len(e["top_logprobs"]) == 3 and e["top_logprobs"][0]["token"] == e["token"]
                assert e["top_logprobs"][0]["logprob"] == e["logprob"] < 0
                assert all(set(t) == {"token", "logprob", "bytes"} for t in e["top_logprobs"])
            assert any(e["bytes"] == [] and e["token"] == "" for e in content) or all(t < 40 for t in stream)
            j0 = (await cl.post("/v1/chat/completions", json=dict(req, logprobs=True))).json()
            assert [e["top_logprobs"] for e in j0["choices"][0]["logprobs"]["content"]] == [[]] * 7
            r = await cl.post("/v1/chat/completions", json=dict(req, logprobs=True, top_logprobs=3, stream=True))
            chunks = [json.loads(x[6:]) for x in r.text.split("\n\n") if x.startswith("data: {")]
            got = [e for c in chunks for e in c["choices"][0].get("logprobs", {"content": []})["content"]]
            assert got == content                                 # streamed entries concatenate to the one-body list
            assert chunks[-1]["choices"][0]["finish_reason"] == "stop" and "logprobs" not in chunks[-1]["choices"][0]
            r0 = await cl.post("/v1/chat/completions", json=dict(req, stream=True))
            assert "logprobs" not in r0.text
            for bad in (dict(req, top_logprobs=2), dict(req, logprobs=True, top_logprobs=21), dict(req, logprobs=True, top_logprobs=-1)):
                assert (await cl.post("/v1/chat/completions", json=bad)).status_code == 422
        eng.shutdown()

    asyncio.run(main())


def test_chat_request_fields():
    r = ChatCompletionRequest(messages=[{"role": "user", "content": "hi"}])
    assert r.logprobs is False and r.top_logprobs is None
    with pytest.raises(Exception):
        ChatCompletionRequest(messages=[], top_logprobs=1)


def test_c_abi_token_logprobs_checks_arguments_without_a_gpu():
    import chirrup_amd
    from chirrup_amd import lib

    hdr = open(os.path.join(ROOT, "include", "chirrup_amd.h")).read()
    assert re.search(r"int rwkv7_token_logprobs\(", hdr)
    assert int(re.search(r"#define\s+CHIRRUP_ABI_VERSION\s+(\d+)", hdr).group(1)) == 4
    if not os.path.exists(chirrup_amd.LIB_PATH):
        chirrup_amd.build()
    L = chirrup_amd.load()
    assert L.chirrup_abi_version() == 4 and "rwkv7_token_logprobs" in lib.SIGNATURES
    f = L.rwkv7_token_logprobs
    p = ctypes.c_void_p(4096)                                  # never dereferenced: validation fails first
    assert f(0, 64, 1, p, None, None, None, p, p, None) == -1           # no rows
    assert f(1, 60, 1, p, None, None, None, p, p, None) == -1           # V % 8
    assert f(1, 65544, 1, p, None, None, None, p, p, None) == -1        # V > 65536
    assert f(1, 64, 21, p, None, None, None, p, p, None) == -1          # K > 20
    assert f(1, 8, 9, p, None, None, None, p, p, None) == -1            # K > V
    assert f(1, 64, -1, p, None, None, None, p, p, None) == -1
    assert f(1, 64, 1, None, None, None, None, p, p, None) == -2        # logits
    assert f(1, 64, 1, p, None, None, None, None, p, None) == -2        # out_lp
    assert f(1, 64, 1, p, None, None, None, p, None, None) == -2        # out_ids with K > 0
    assert f(1, 64, 1, ctypes.c_void_p(4098), None, None, None, p, p, None) == -3


@pytest.mark.skipif(shutil.which(HIPCC) is None and not os.path.exists(HIPCC), reason="no hipcc")
def test_token_logprobs_kernel_has_no_scratch_spills():
    """The compiler's resource report (the method of test_kernel_budget_cpu.py): the row's 32 packed key pairs stay in registers."""
    csrc = os.path.join(ROOT, "chirrup_amd", "csrc")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
             "-Rpass-analysis=kernel-resource-usage", "-c"]
    out = subprocess.run([HIPCC] + flags + [os.path.join(csrc, "sampler.hip"), "-o", os.devnull], capture_output=True, text=True, cwd=csrc)
    assert out.returncode == 0, out.stderr[-2000:]
    rep, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            continue
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and cur:
            rep[cur] = int(m.group(1))
    hits = {n: s for n, s in rep.items() if "token_logprobs_kernel" in n}
    assert hits and all(s == 0 for s in hits.values()), hits
