"""plan_forward: which kernels a fused forward runs for a given (rows, T, C, dtype, knobs), decided on the host alone."""
import os
import types

import pytest
import torch

import chirrup_amd
from chirrup_amd import rwkv7
from chirrup_amd.rwkv7 import plan_forward


@pytest.fixture(scope="module", autouse=True)
def _library():
    # the mm8 ffn.key decision asks the library's host-side helpers (ops.mm8_fused_split_ok)
    if not os.path.exists(chirrup_amd.LIB_PATH):
        chirrup_amd.build()
    chirrup_amd.load()


def knobs(C, **over):
    """RWKV_x070's knob defaults at width C on a full-size device (chain_tmix_gemms: >= 192 CUs)."""
    k = types.SimpleNamespace(
        skinny_ffn_value=True, skinny_min_rows=1, skinny_min_embd=0, skinny_lora_up=True, tune_prefill_gemms=True,
        mm8_prefill_dequant=True, mm8_fused_key=True, mm8_pair_key=True, mm8_pair_max_rows=16, lora_up_row_halves=True,
        group_tmix_gemms=True, chain_tmix_gemms=True, chain_min_rows=1 if C >= 2560 else 129, skinny_rkv=False,
        skinny_wide_rows=1, skinny_head=True, skinny_att_out=True, skinny_ffn_key=True, fuse_tmix_core=True, split_tmix_min_T=32,
        gemm_splits={"rkv": 0, "att_out": 0, "ffn_key": 0, "ffn_value": 0}, row_halves_min_rows=128,
        gemm_row_halves={"rkv": True, "att_out": True, "ffn_key": True, "ffn_value": False}, keep_row_major=True,
        ffn_dtype=torch.float16, att_dtype=torch.float16)
    for n, v in over.items():
        setattr(k, n, v)
    return k


def layer(ffn8=False, att8=False, sparse=False, tiled=True):
    """_Layer's tiling facts: tile images of the fp16 matrices, uint8 tilings, the bsz-1 sparse rows."""
    t = object() if tiled else None
    return types.SimpleNamespace(rkv_t=None if att8 else t, lora2_t=t, a8_tiled=att8 and tiled, f8_tiled=ffn8 and tiled,
                                 f_V_rows=object() if sparse else None)


def plan(C, rows, T=1, lw=None, **over):
    return plan_forward(knobs(C, **over), rows, T, C, lw if lw is not None else layer())


def test_knob_defaults_match_the_model():
    from chirrup_amd.synth import make_state_dict

    m = rwkv7.RWKV_x070(types.SimpleNamespace(vocab_size=256, head_size=64, MODEL_NAME="unused"),
                        state_dict=make_state_dict(1, 128, 256, seed=0), device="cpu")
    want = vars(knobs(128))
    assert {n: getattr(m, n) for n in want} == want


def test_decode_full_width_chain():
    p = plan(4096, 200)
    assert (p.hw, p.use_parts, p.fuse_core) == (True, True, True)
    assert p.row_halves == {"rkv": True, "att_out": True, "ffn_key": True, "ffn_value": False}
    assert (p.rkv, p.lora, p.side) == ("chain", "launch", False)
    assert (p.att_out, p.ffn_key, p.ffn_value, p.head) == ("ring", "ring", "ring", "ring")


def test_decode_narrow_below_chain_min_rows_is_grouped():
    p = plan(2048, 32)
    assert (p.rkv, p.lora, p.side) == ("grouped", "grouped", False)
    assert not any(p.row_halves.values())


def test_chain_off_is_grouped():
    assert (plan(4096, 200, chain_tmix_gemms=False).rkv, plan(4096, 200, chain_tmix_gemms=False).lora) == ("grouped", "grouped")
    assert plan(4096, 200, chain_tmix_gemms=False, group_tmix_gemms=False).lora == "bmm_ring"
    assert plan(4096, 200, group_tmix_gemms=False, skinny_lora_up=False).lora == "bmm_baddbmm"


def test_prefill_2500_rows_library():
    p = plan(4096, 2500, T=100)
    assert (p.hw, p.use_parts, p.fuse_core) == (False, False, False)
    assert (p.rkv, p.lora, p.side) == ("mm3", "per_problem", True)
    assert (p.att_out, p.ffn_key, p.ffn_value, p.head) == ("library", "mm_nt", "mm_nt", "library")


def test_prefill_300_rows_batched():
    p = plan(4096, 300, T=100)
    assert (p.rkv, p.lora, p.side, p.ffn_key, p.ffn_value) == ("bmm", "per_problem", True, "mm_nt", "matmul")


def test_decode_gemms_with_short_chunks():
    p = plan(4096, 64, T=16)
    assert (p.hw, p.fuse_core, p.rkv, p.att_out, p.ffn_key, p.ffn_value) == (True, True, "chain", "ring", "ring", "ring")
    assert plan(2048, 64, T=16).rkv == "grouped"
    assert plan(4096, 64, T=32).fuse_core is False


def test_sparse_bsz1():
    assert plan(4096, 1, lw=layer(sparse=True)).ffn_value == "sparse"
    assert plan(4096, 1).ffn_value == "ring"
    assert plan(4096, 2, lw=layer(sparse=True)).ffn_value == "ring"


@pytest.mark.parametrize("rows,key", [(200, "mm8_fused"), (8, "mm8_pair"), (32, "mm8_partial")])
def test_mm8_ffn_key_forms(rows, key):
    p = plan(4096, rows, lw=layer(ffn8=True), ffn_dtype=torch.int8)
    assert (p.hw, p.use_parts, p.ffn_key, p.ffn_value) == (True, False, key, "mm8_parts")
    assert (p.rkv, p.att_out, p.head) == ("chain", "ring", "ring")


def test_mm8_pair_off():
    assert plan(4096, 8, lw=layer(ffn8=True), ffn_dtype=torch.int8, mm8_pair_key=False).ffn_key == "mm8_partial"


def test_mm8_ffn_prefill():
    p = plan(4096, 2500, T=100, lw=layer(ffn8=True), ffn_dtype=torch.int8)
    assert (p.ffn_key, p.ffn_value) == ("mm8_dequant", "mm8_dequant")
    p = plan(4096, 2500, T=100, lw=layer(ffn8=True), ffn_dtype=torch.int8, mm8_prefill_dequant=False)
    assert (p.ffn_key, p.ffn_value) == ("mm8", "mm8")


def test_mm8_ffn_chunks_need_single_tokens():
    p = plan(4096, 64, T=16, lw=layer(ffn8=True), ffn_dtype=torch.int8)
    assert (p.hw, p.ffn_key, p.ffn_value) == (True, "mm8", "mm8")


def test_mm8_fused_att_output_ignores_skinny_wide_rows():
    # the fused uint8 att.output never checked skinny_wide_rows; its partials buffer is allocated for it either way
    lw = layer(ffn8=True, att8=True)
    assert plan(4096, 32, lw=lw, ffn_dtype=torch.int8, att_dtype=torch.int8, skinny_wide_rows=64).att_out == "mm8_fused"
    assert plan(4096, 32, skinny_wide_rows=64).att_out == "library"


def test_mm8_all_decode():
    lw = layer(ffn8=True, att8=True)
    p = plan(4096, 200, lw=lw, ffn_dtype=torch.int8, att_dtype=torch.int8)
    assert (p.rkv, p.lora, p.side) == ("chain_mm8", "launch", False)
    assert (p.att_out, p.ffn_key, p.ffn_value, p.head) == ("mm8_fused", "mm8_fused", "mm8_parts", "mm8")
    p = plan(4096, 64, T=16, lw=lw, ffn_dtype=torch.int8, att_dtype=torch.int8)
    assert (p.rkv, p.lora, p.att_out) == ("mm8", "grouped", "mm8")
    p = plan(4096, 2500, T=100, lw=lw, ffn_dtype=torch.int8, att_dtype=torch.int8)
    assert (p.rkv, p.lora, p.side, p.att_out, p.head) == ("mm8", "per_problem", True, "mm8", "mm8")


def test_tile_image_only_prefill():
    # library GEMMs (not hw) of a model without row-major copies: the forward rebuilds them from the tile images (_row_major)
    p = plan(4096, 2500, T=100, keep_row_major=False)
    assert (p.hw, p.rkv, p.head) == (False, "mm3", "ring")
    assert plan(4096, 2500, T=100).head == "library"


def test_without_tile_images():
    p = plan(4096, 200, lw=layer(tiled=False))
    assert (p.rkv, p.lora, p.att_out, p.ffn_value, p.head) == ("grouped", "grouped", "ring", "ring", "ring")
