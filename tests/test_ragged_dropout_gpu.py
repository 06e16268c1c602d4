"""Skip-padding training with dropout against a masked fp64 oracle: stlt_train_forward / stlt_train_backward with STLT_FLAG_SKIP_PADDING
and hidden_dropout_prob > 0 — logits and EVERY live parameter's gradient — against tests/ragged_restated.py applying the same counter-based
masks, drawn per compacted row, under torch autograd.  The backward kernels store no mask: they draw it again from (seed, site, element
index), so a forward / backward disagreement about the index leaves finite, seeded, reproducible — and wrong — gradients; this comparison
is what notices (tests/test_ragged_dropout_cpu.py shows that the padded-position index alone moves the logits by > 1000 x the bounds here).

Cases, shapes and references: tests/ragged_cases.py (CASES; two spatial + two temporal layers each, so each tower has a full layer
and, where the row counts allow, a tail layer, and the per-layer site stride of 8 is exercised).  The kernels each case reaches, read from the
dispatch in csrc/train.hip (qkv_attention_train, layer_forward, layer_backward(_tail)), attn.hip (launch_attn_ragged), attn_any.hip,
backward.hip (launch_attn_bwd) and attn_bwd16.hip (launch_attn_bwd16_ragged):

  every case  embed_rows / frames_embed kernels with the ragged index (SITE_EMBED / SITE_FRAMES over compacted rows), add_ln_kernel
              (dropout1 / dropout2); backward: ln_bwd kernels (the masks of dropout1 / dropout2 and of both embedding sites).  The FFN
              hidden site (width 4d): at hidden sizes 64 - 256 (A, B, C, E, F, G) the small-tile products carry it in their epilogues both
              ways — gemm16 with STLT_ACT_GELU_KEEP forward, its input-gradient build with STLT_ACT_GELU_BWD backward; at hidden size 32
              (D) the forward is product + gelu_fwd_kernel and the backward gemm.hip's large-tile product with the GELU_BWD epilogue; at
              hidden size 48 (H) neither product takes it: gelu_fwd_kernel and gelu_bwd_colsum_kernel.  In a tail layer all of these take
              drop_rows = the picked rows (the frames' CLS rows / the clips' last rows).  Every case asserts its routes on the library's
              launch recorder (ragged_cases.assert_routes), so a dispatch change cannot leave this table stale.
  A (p 0.1, 0.5)  head dim 64: forward attn_core_kernel<VARLEN> (attn.hip) in both towers; backward attn_bwd16_kernel<2, RAGGED>: spatial
              groups of fpg = 8 whole frames (<= 32 rows), temporal groups = clips (<= 16 rows); both towers end in a tail layer.
  B           CLS-only frames: as many tokens as frames, so 2 * frames > tokens — no spatial tail layer (the CLS rows are gathered after a
              full last layer, the reverse sweep scatters their gradient); one-row spatial segments.  Kernels as A.
  C           T = 1, lengths 1: 2 * clips > frames — no temporal tail layer (last rows gathered / scattered); the spatial tower keeps its
              tail (11 tokens, 4 frames).  Kernels as A, fpg = 10.
  D (p 0.3)   head dim 8: attn_any_fwd_kernel with segments, attn_any_bwd_kernel with groups (attn_any.hip, vector ALU) in both towers,
              hidden size 32; both tails.
  E           N = 36 > 32: fpg = 1, spatial backward groups are single frames of up to 36 rows: attn_bwd16_kernel<3, RAGGED>; the forward
              tile of 32 queries walks two key tiles; slots masked inside the frames (key position != slot number).
  F           T = 70 > 64 with a full-length clip: the temporal backward is attn_bwd_long_kernel with grp_ptr (backward.hip: one block per
              clip and head, keys streamed in tiles of 32), the temporal forward walks three key tiles per query tile; hidden size 64, one head.
              1.5 tokens per frame: no spatial tail layer.
  G           A's batch with slot 2 masked and slot 3 real in two frames, and frame 5 of the full-length clip masked with real frames behind
              it (csrc/ragged.hip accepts both holes: its contract is only that slot 0 of a real frame and frame lengths-1 are real, and the
              Python side adds no check of its own): the key position inside the segment is neither the slot nor the frame number.
  H           hidden size 48, head dim 12 (d % 32 != 0): stlt_ffn_hidden_bwd (blocks.hip) runs a plain input-gradient product and then
              gelu_bwd_colsum_kernel, which redraws the FFN-hidden mask at drop_rows[m] * 4d + c — in the full layers and in both tail
              layers; forward gelu_fwd_kernel (drop_index); attention on attn_any.hip as D.
  A, frozen   gelu_bwd_kernel (drop_index) runs where no linear1.bias gradient is asked for: case A with the four linear1 biases frozen
              (test_stand_alone_gelu_backward_when_the_ffn_bias_is_frozen).

The ragged form of backward.hip's attn_bwd_kernel (plain FMA, groups of <= 64 rows at head dim 64) is reached by no default dispatch: the
MFMA kernel takes every such group.  STLT_ATTN_BWD16=0 — read once per process — routes to it, so a child process runs cases A, E and G
with that switch and asserts on the recorder that the FMA kernel ran (test_fma_ragged_attention_backward_draws_the_same_masks,
tests/ragged_dropout_child.py)."""
import os
import subprocess
import sys

import pytest

from ragged_cases import CASES, assert_routes, build_model, check_step, logit_bound, padded_reference, ragged_reference, train_step

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", sorted(CASES))
def test_skip_padding_training_with_dropout_matches_the_ragged_masked_oracle(pkg, name):
    """The table of the module docstring, one case each: the step against the oracle, then the kernels it ran against the table."""
    m = build_model(pkg, name)
    check_step(f"{name} ragged", name, train_step(m, name, True), ragged_reference(name), logit_bound(name))
    assert_routes(pkg, m, name)


def test_padded_and_ragged_steps_with_dropout_alternate_on_the_same_buffers(pkg):
    """Case A at p = 0.1: a ragged step, then a padded step on the same model, tape and scratch — which must still match the padded oracle
    under padded-position masks — then a ragged step again.  Stale rows or a stale index from the other schedule must not leak."""
    name = "A-p0.1"
    m = build_model(pkg, name)
    check_step("alternation ragged 1", name, train_step(m, name, True), ragged_reference(name), logit_bound(name))
    check_step("alternation padded", name, train_step(m, name, False), padded_reference(name), logit_bound(name))
    check_step("alternation ragged 2", name, train_step(m, name, True), ragged_reference(name), logit_bound(name))


def test_stand_alone_gelu_backward_when_the_ffn_bias_is_frozen(pkg):
    """Case A at p = 0.1 with every linear1.bias frozen: the sweep is asked for no lin1 bias gradient, so stlt_ffn_hidden_bwd (blocks.hip)
    leaves the fused epilogue for a plain product + gelu_bwd_kernel, whose mask index is drop_index(): row * 4d + e, the row taken from
    drop_rows in the tail layers.  Every other gradient is still the oracle's; the frozen biases get none."""
    name = "A-p0.1"
    m = build_model(pkg, name)
    frozen = [k for k, p in m.named_parameters() if k.endswith("linear1.bias") and "encoder_layer." not in k]
    assert len(frozen) == 4
    params = dict(m.named_parameters())
    for k in frozen:
        params[k].requires_grad_(False)
    check_step("A-p0.1 ragged, linear1.bias frozen", name, train_step(m, name, True), ragged_reference(name), logit_bound(name), frozen=frozen)
    assert_routes(pkg, m, name, ffn_bwd="gelu_bwd")


def test_fma_ragged_attention_backward_draws_the_same_masks():
    """backward.hip's attn_bwd_kernel in its ragged form (groups of whole segments, masks indexed by the key's position in the query's
    segment) is behind STLT_ATTN_BWD16=0, which the library reads once per process: a child process (tests/ragged_dropout_child.py)
    runs cases A (32- and 16-row groups), E (36-row groups) and G (holes) with it, holds them to the same references and bounds, and
    asserts on the launch recorder that both towers' attention backward ran on that kernel."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ragged_dropout_child.py")
    r = subprocess.run([sys.executable, child, "A-p0.1", "E", "G"], capture_output=True, text=True, timeout=600, env=dict(os.environ, STLT_ATTN_BWD16="0"))
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
