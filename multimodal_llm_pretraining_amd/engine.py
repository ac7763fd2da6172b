"""Forward / backward of one micro-batch of the ViT → projector → Pythia step,
written explicitly over the libmmpt HIP kernels (no torch.autograd on the hot
path, no ATen compute).

Mirrors, op for op, the arithmetic HF runs inside
`Trainer.training_step` → `model(**inputs).loss` → `backward()` for
LlavaForConditionalGeneration(ViT, GPTNeoX) / GPTNeoXForCausalLM under bf16
autocast (reference call stack: SURVEY.md §3.2; math:
tf:models/gpt_neox/modeling_gpt_neox.py:180-384, tf:models/vit/modeling_vit.py:
42-300, tf:models/llava/modeling_llava.py:87-248, tf:loss/loss_utils.py:32-68):

* residual streams fp32, LayerNorm fp32 → bf16 GEMM operand (fused cast);
* GEMMs bf16 × bf16 → fp32 accumulate → bf16 out, bias/GELU/residual fused in
  the epilogue; weight grads rounded to bf16 then accumulated in fp32
  (autocast's bf16 grad → fp32 .grad);
* attention via the flash kernels, partial RoPE in place on the fused qkv;
* cross-entropy fused fwd+bwd over bf16 logits (fp32 math), dlogits in place.

A vision-only classifier (ModelConfig.classifier: ViTForImageClassification,
tf:models/vit/modeling_vit.py) runs the same ViT encoder, then the final LayerNorm on the CLS
rows, the classifier GEMM and the cross entropy over one row per image (_cls_forward /
_cls_backward).

A masked LM (TextConfig.arch "roberta": RobertaForMaskedLM, tf:models/roberta/modeling_roberta.py)
is a post-LN encoder: LayerNorm after each residual add (include/mmpt.h K20), learned positions,
the MLM head on the labelled rows (_roberta_forward / _roberta_backward).

A ConvNeXt classifier (ModelConfig.convnext: ConvNextForImageClassification,
tf:models/convnext/modeling_convnext.py) keeps its activations channels-last: rows (b, y, x),
columns c.  The 7x7 depthwise conv, the layer-scale residual, the pool and the 2x2 patch
permutations are include/mmpt.h K21; every 1x1 conv, the 4x4 stem and the 2x2 downsample are
GEMMs over those rows (_convnext_forward / _convnext_backward).

A Mamba language model (TextConfig.arch "mamba": MambaForCausalLM,
tf:models/mamba/modeling_mamba.py) has no attention: each block is an RMSNorm, five GEMMs, the
causal conv and the selective scan of include/mmpt.h K22, with the arithmetic of the reference's
fused path; around its blocks it is the causal-LM step (_causal_forward / _causal_backward).

Every family's step runs in one frame: _begin (the prologue), the family's body, _loss (cross
entropy + sum, and what a forward without gradients keeps: nothing); _begin_backward (the head's
cache entry, dlogits scaled), the body, _finish.  Engine.__init__ picks the family once.
"""

from __future__ import annotations

import os
from typing import NamedTuple

import numpy as np
import torch

from . import kernels as K
from .config import ModelConfig
from .droppath import kept_indices_of
from .params import ParamStore

BF16 = torch.bfloat16
F32 = torch.float32


def rope_tables(hidden: int, heads: int, rotary_pct: float, theta: float, seq: int):
    """cos/sin [seq][rot] in fp32, computed on the CPU exactly as
    tf:modeling_gpt_neox.py:76-110 does (so the oracle and the GPU share bits)."""
    head_dim = hidden // heads
    dim = int(head_dim * rotary_pct)
    inv_freq = 1.0 / (theta ** (torch.arange(0, dim, 2, dtype=torch.int64).float() / dim))
    pos = torch.arange(seq).float()
    freqs = pos[:, None] * inv_freq[None, :]
    emb = torch.cat((freqs, freqs), dim=-1)
    return emb.cos().contiguous(), emb.sin().contiguous()


def rope_tables_llama3(head_dim: int, theta: float, scaling, seq: int):
    """Llama-3 rotary tables (transformers modeling_rope_utils.py _compute_llama3_parameters:
    inverse frequencies rescaled by `factor` below the low-frequency wavelength and smoothly
    interpolated in between; LlamaRotaryEmbedding.forward: fp32 outer product, cat, cos/sin,
    attention factor 1), computed on the CPU with HF's own op sequence."""
    import math

    inv_freq = 1.0 / (theta ** (torch.arange(0, head_dim, 2, dtype=torch.int64).float() / head_dim))
    if scaling is not None:
        factor, low, high, old = scaling
        low_wl, high_wl = old / low, old / high
        wavelen = 2 * math.pi / inv_freq
        inv_l = torch.where(wavelen > low_wl, inv_freq / factor, inv_freq)
        smooth = (old / wavelen - low) / (high - low)
        smoothed = (1 - smooth) * inv_l / factor + smooth * inv_l
        medium = ~(wavelen < high_wl) * ~(wavelen > low_wl)
        inv_freq = torch.where(medium, smoothed, inv_l)
    pos = torch.arange(seq).float()
    with torch.autocast("cpu", enabled=False):
        freqs = (inv_freq[None, :, None] @ pos[None, None, :]).transpose(1, 2)[0]
        emb = torch.cat((freqs, freqs), dim=-1)
        return emb.cos().contiguous(), emb.sin().contiguous()


def sort_segments(ids: np.ndarray, rows: np.ndarray):
    """(seg_id, seg_off, perm) int32 for mmpt_embed_bwd: `rows` stably sorted by ids[row],
    one segment per distinct id (perm[seg_off[s]:seg_off[s+1]] all have id seg_id[s])."""
    perm = rows[np.argsort(ids[rows], kind="stable")]
    sid = ids[perm]
    starts = np.concatenate(([0], np.flatnonzero(np.diff(sid)) + 1)) if sid.size else \
        np.zeros(0, np.int64)
    seg_off = np.concatenate((starts, [perm.size]))
    return tuple(np.ascontiguousarray(a, dtype=np.int32) for a in (sid[starts], seg_off, perm))


# Hidden-dropout site ids (mmpt_dropout_*'s 64-bit `site`): | step 32 | rank 16 | unit 12 | k 4 |
# bits.  unit: 0 = the text embedding, 1 + i = text layer i, VISION_UNIT = the ViT embedding,
# VISION_UNIT + 1 + i = ViT layer i (so at most 2047 layers a side); k: the site inside the
# unit (a layer: 0 = after the attention output projection, 1 = after the MLP, 2 = the
# attention probabilities — the site of the mmpt_attention_drop_* calls, which share the seed;
# unit 0 also has k = 4 = the NEFTune noise on the token embedding, Engine.neftune_alpha).
# ConvNeXt: VISION_UNIT + 1 + j = block j counted over all stages, k = 3 = its drop-path bits
# (element b = sample b; the blocks have no other site).
SITE_STEPS, SITE_RANKS, SITE_UNITS, SITE_KS = 1 << 32, 1 << 16, 1 << 12, 1 << 4
VISION_UNIT = SITE_UNITS // 2


def dropout_site(step: int, rank: int, unit: int, k: int) -> int:
    """The 64-bit site of a dropout mask: micro-step counter, data-parallel rank, unit, site
    within the unit, each in its own bit field — injective over 0 <= step < 2^32, 0 <= rank <
    2^16, 0 <= unit < 2^12, 0 <= k < 2^4; anything outside raises ValueError."""
    for name, v, n in (("step", step, SITE_STEPS), ("rank", rank, SITE_RANKS),
                       ("unit", unit, SITE_UNITS), ("k", k, SITE_KS)):
        if not 0 <= v < n:
            raise ValueError(f"dropout_site: {name} {v} outside [0, {n})")
    return (step << 32) | (rank << 16) | (unit << 4) | k


class AttnLayout(NamedTuple):
    """Where the heads sit in a row of the fused qkv GEMM output, in elements (the layout arguments
    of mmpt_attention_gqa_fwd): q head j at j * head_stride, its kv head at k_offset / v_offset +
    (j // (heads / kv_heads)) * head_stride."""
    heads: int
    kv_heads: int
    head_dim: int
    head_stride: int
    k_offset: int
    v_offset: int
    causal: bool

    @classmethod
    def neox(cls, t):
        """GPTNeoX: q | k | v interleaved per head."""
        H, D = t.heads, t.head_dim
        return cls(H, H, D, 3 * D, D, 2 * D, True)

    @classmethod
    def gqa(cls, t):
        """Llama: every q head, then the kv_heads k heads, then the v heads."""
        H, Hk, D = t.heads, t.n_kv, t.head_dim
        return cls(H, Hk, D, D, H * D, (H + Hk) * D, True)

    @classmethod
    def planar(cls, c):
        """ViT / RoBERTa: q | k | v, each `hidden` wide; bidirectional."""
        return cls(c.heads, c.heads, c.head_dim, c.head_dim, c.hidden, 2 * c.hidden, False)


class Batch:
    """A micro-batch staged in HBM with its index bookkeeping precomputed (label shift,
    loss-row compaction, image-token map, the embedding backward's id segments): the step
    reads only device memory.

    Host tensors (what a data loader yields, ideally pinned): the bookkeeping that sizes
    kernels (label count, scored rows, image-slot count) is computed from the host copy, the
    id segments are sorted on the device (`mmpt_embed_segments`), and every host-to-device
    copy is asynchronous on the current stream — building a Batch never waits for the GPU,
    so it can sit inside the timed step like the reference's `_prepare_inputs`
    (src/benchmarking/utils.py:61-63 → Trainer.training_step).  Device tensors are accepted
    too; the counts then cost one device synchronisation.

    Padded batches (`attention_mask` with zeros, right-padded as the reference's LlavaCollator
    pads — src/data/llava_data.py:169-185): the pad positions are DROPPED here.  Labels under
    the mask are forced to -100 and the label shift is done in the padded [B, S] layout (the
    last real token of a row gets no label); then ids, shifted labels, the loss rows, the
    image-token map and the embedding-backward segments are all built over the T = Σ lens
    valid tokens, packed sequence after sequence.  `cu_seqlens` (int32 [B + 1] row offsets) and
    `pos` (int32 [T], the position of each token inside its sequence) carry the geometry to
    the varlen attention and the positional rope; both are None on the dense path (no mask,
    or a mask without zeros), which is then object for object what it was without the
    argument.  B stays the number of rows, S the padded width.

    Packed rows (`position_ids`, int [B, S] in the HF packing convention — what
    DataCollatorWithFlattening and data.pack_collate yield): inside the valid part of a row every
    entry is the previous one + 1 or 0, each row starts at 0, and a 0 starts a new document.  The
    text-only causal LMs take it (GPTNeoX, Llama, Mamba).  When some row restarts after column 0
    the batch takes the same varlen form with one sequence per DOCUMENT, in row-major order:
    `lens` / `cu_seqlens` ([n_seq + 1]) / `pos` / `max_len` describe the documents, `n_seq =
    len(lens)` (B on every other path), and the label shift is done per document — the last token
    of a document gets no target, so nothing is trained to predict the next document's first
    token; a one-token document carries no label.  Trailing pads marked by `attention_mask` are
    dropped as above and `position_ids` under them is ignored.  Without a restart the argument
    changes nothing.  For Mamba `scan_tables` (kernels.ScanTables: the scan's chunk offsets) is
    staged with the rest; a padded Mamba batch without `position_ids` stays refused.

    Masked-LM batches (TextConfig.arch "roberta"): no label shift — the label of row r is the
    target of row r — and `pos_ids` (int64 [T]): HF's create_position_ids_from_input_ids over the
    padded [B, S] ids, cumsum(id != pad_id) * (id != pad_id) + pad_id, so an id equal to pad_id
    inside a sequence sits at position pad_id and does not advance the count; the positions of the
    valid tokens do not depend on dropped right pads.  `pos_segments` are the position table's
    embedding-backward segments (keyed by position id); both tables skip pad_id, their
    padding_idx.

    Image batches (a vision-only classifier, ModelConfig.classifier): `input_ids` is None,
    `pixel_values` is [B, C, S, S] and `labels` [B] holds one class per image, each in
    [0, num_classes).  num_items = B; S / T count the ViT tokens (patches + CLS)."""

    def __init__(self, cfg: ModelConfig, input_ids: torch.Tensor | None, labels: torch.Tensor,
                 pixel_values: torch.Tensor | None, device: torch.device, stream=None,
                 attention_mask: torch.Tensor | None = None,
                 position_ids: torch.Tensor | None = None):
        """stream: stage on this (copy) stream instead of the current one — the copies and
        the segment sort then overlap the compute stream's work; `use(stream)` (called by
        Engine.forward) orders the consumer after them."""
        device = torch.device(device)
        if position_ids is not None and (cfg.classifier or cfg.multimodal or cfg.text.roberta):
            raise ValueError("position_ids (packed documents) is taken by the text-only causal "
                             "language models (GPTNeoX, Llama, Mamba), not by multimodal, RoBERTa "
                             "or classifier configs")
        if cfg.classifier:
            self._init_images(cfg, input_ids, labels, pixel_values, device, stream, attention_mask)
            return
        if input_ids is None:
            raise ValueError("a language model needs input_ids")
        self.B, self.S = input_ids.shape
        # the width of input_ids as the batch arrived (padded / flattened / with the image
        # slots): NEFTune's magnitude is alpha / sqrt(S_in * hidden), HF's output.size(1)
        self.S_in = self.S
        cfg.text.check_seq(self.S)
        self.pos_ids, self.pos_segments = None, ()
        if cfg.multimodal and pixel_values is None:
            raise ValueError("multimodal model needs pixel_values")
        self.T, self.max_len = self.B * self.S, self.S
        self.lens = [self.S] * self.B
        self.cu_seqlens = self.pos = self.scan_tables = None
        mask = self._check_mask(attention_mask)
        restart = None if position_ids is None else self._check_positions(position_ids)
        self.n_seq = len(self.lens)
        if mask is not None and cfg.text.mamba and position_ids is None:
            raise ValueError("arch 'mamba': attention_mask has zeros — padded batches are taken "
                             "with position_ids only (data.pack_collate yields them); without "
                             "them the scan and the conv run over whole rows")
        self._ready = None
        if stream is not None and device.type == "cuda":
            with torch.cuda.stream(stream):
                self._stage(cfg, input_ids, labels, pixel_values, device, mask, restart)
            self._ready = torch.cuda.Event()
            self._ready.record(stream)
        else:
            self._stage(cfg, input_ids, labels, pixel_values, device, mask, restart)

    def _init_images(self, cfg, input_ids, labels, pixel_values, device, stream, attention_mask):
        v = cfg.vision if cfg.convnext is None else cfg.convnext
        if input_ids is not None or attention_mask is not None:
            raise ValueError("an image classifier takes pixel_values and labels, not input_ids / "
                             "attention_mask")
        if pixel_values is None:
            raise ValueError("an image classifier needs pixel_values")
        want = (v.channels, v.image, v.image)
        if pixel_values.dim() != 4 or tuple(pixel_values.shape[1:]) != want:
            raise ValueError(f"pixel_values shape {tuple(pixel_values.shape)} != [B, "
                             f"{v.channels}, {v.image}, {v.image}]")
        # S / T count the rows of the first residual stream: ViT tokens, or ConvNeXt stem pixels
        self.B = pixel_values.shape[0]
        self.S = v.num_patches + 1 if cfg.convnext is None else v.side(0) ** 2
        if tuple(labels.shape) != (self.B,):
            raise ValueError(f"labels shape {tuple(labels.shape)} != [{self.B}] (one class per "
                             "image)")
        self.T, self.max_len = self.B * self.S, self.S
        self.lens = [self.S] * self.B
        self.n_seq = self.B
        self.cu_seqlens = self.pos = self.scan_tables = None
        self._ready = None
        if stream is not None and device.type == "cuda":
            with torch.cuda.stream(stream):
                self._stage_images(cfg, labels, pixel_values, device)
            self._ready = torch.cuda.Event()
            self._ready.record(stream)
        else:
            self._stage_images(cfg, labels, pixel_values, device)

    def _stage_images(self, cfg, labels, pixel_values, device):
        lab = labels.to(torch.int64)
        if lab.device.type == "cpu":  # validated on the host copy: no device synchronisation
            _check_labels(lab.numpy(), cfg.num_classes)
        elif lab.numel():
            _check_labels(torch.stack((lab.min(), lab.max())).cpu().numpy(), cfg.num_classes)
        self.num_items = self.B
        self.ids = self.img_map = self.loss_rows = self.loss_map = None
        self.labels = self.loss_labels = _to(lab, device, torch.int64)
        self.pixels = _to(pixel_values, device, F32)
        self.segments = ()
        self.pos_ids, self.pos_segments = None, ()

    def _check_mask(self, attention_mask):
        """None for the dense path (no mask, or no zero in it); else the host bool [B, S] mask,
        validated as right-padded, with lens / T / max_len set from it."""
        if attention_mask is None:
            return None
        if tuple(attention_mask.shape) != (self.B, self.S):
            raise ValueError(f"attention_mask shape {tuple(attention_mask.shape)} != input_ids "
                             f"shape {(self.B, self.S)}")
        m = (attention_mask != 0)
        if bool(m.all()):
            return None
        m = m.cpu().numpy()
        lens = m.sum(1)
        for b in range(self.B):
            if lens[b] == 0:
                raise ValueError(f"attention_mask row {b} is empty (no valid token)")
            if not m[b, :lens[b]].all():
                first, last = np.flatnonzero(m[b])[[0, -1]]
                if last - first + 1 == lens[b] and last == self.S - 1:
                    raise ValueError(f"attention_mask row {b} is left-padded; only right "
                                     "padding is supported")
                raise ValueError(f"attention_mask row {b} has holes; only right padding (ones "
                                 "then zeros) is supported")
        self.lens = [int(x) for x in lens]
        self.T, self.max_len = int(lens.sum()), int(lens.max())
        return torch.from_numpy(m)

    def _check_positions(self, position_ids):
        """None when no row restarts after column 0 (the argument then changes nothing); else the
        host bool [B, S] map of the columns > 0 at which a document starts, with lens / T /
        max_len set to the documents' (row-major).  The valid part of row b is its first
        lens[b] columns (the whole row without a padding mask)."""
        if tuple(position_ids.shape) != (self.B, self.S):
            raise ValueError(f"position_ids shape {tuple(position_ids.shape)} != input_ids shape "
                             f"{(self.B, self.S)}")
        if position_ids.is_floating_point() or position_ids.dtype == torch.bool:
            raise ValueError(f"position_ids must be an integer tensor, got {position_ids.dtype}")
        p = position_ids.detach().to("cpu", torch.int64).numpy()
        restart = np.zeros((self.B, self.S), bool)
        docs = []
        for b in range(self.B):
            n = self.lens[b]
            r = p[b, :n]
            if r[0] != 0:
                raise ValueError(f"position_ids row {b} column 0 is {int(r[0])}: every row starts "
                                 "at 0")
            bad = np.flatnonzero((r[1:] != r[:-1] + 1) & (r[1:] != 0))
            if bad.size:
                c = int(bad[0]) + 1
                raise ValueError(f"position_ids row {b} column {c} is {int(r[c])} after "
                                 f"{int(r[c - 1])}: neither the previous position + 1 nor a "
                                 "restart at 0")
            starts = np.flatnonzero(r == 0)
            restart[b, starts[1:]] = True
            docs.extend(int(x) for x in np.diff(np.concatenate((starts, [n]))))
        if not restart.any():
            return None
        if len(docs) > 65535:
            raise ValueError(f"position_ids marks {len(docs)} documents; at most 65535 sequences "
                             "in a batch")
        self.lens = docs
        self.T, self.max_len = sum(docs), max(docs)
        return torch.from_numpy(restart)

    def _stage(self, cfg, input_ids, labels, pixel_values, device, mask=None, restart=None):
        if input_ids.device.type == "cpu" and labels.device.type == "cpu":
            self._from_host(cfg, input_ids, labels, device, mask, restart)
        else:
            self._from_device(cfg, input_ids, labels, device, mask, restart)
        if mask is not None or restart is not None:
            cu = np.concatenate(([0], np.cumsum(self.lens))).astype(np.int32)
            pos = np.concatenate([np.arange(n, dtype=np.int32) for n in self.lens])
            self.cu_seqlens = _to(torch.from_numpy(cu), device, torch.int32)
            self.pos = _to(torch.from_numpy(pos), device, torch.int32)
            if cfg.text.mamba and device.type == "cuda":  # the varlen scan's chunk offsets
                self.scan_tables = K.scan_tables(self.lens, device)
        self.pixels = None
        if cfg.multimodal:
            self.pixels = _to(pixel_values, device, F32)
        self.segments = self._segments(cfg, device)
        if cfg.text.roberta:
            self.pos_segments = self._segments(cfg, device, self.pos_ids, cfg.text.max_positions)

    def use(self, stream) -> None:
        """Order `stream` after the staging stream and hand the staged tensors to it (the
        caching allocator then frees them only after `stream`'s use)."""
        if self._ready is None:
            return
        stream.wait_event(self._ready)
        for t in (self.ids, self.labels, self.loss_rows, self.loss_labels, self.loss_map,
                  self.img_map, self.pixels, self.cu_seqlens, self.pos, self.pos_ids,
                  *self.segments, *self.pos_segments,
                  *((self.scan_tables.cu_seqlens, self.scan_tables.cu_chunks)
                    if self.scan_tables is not None else ())):
            if t is not None:
                t.record_stream(stream)
        self._ready = None

    def _from_host(self, cfg, input_ids, labels, device, mask=None, restart=None):
        ids = input_ids.reshape(-1).to(torch.int64)
        lab = labels.to(torch.int64)
        if mask is not None:  # HF's Llava loss drops the labels under the mask
            lab = lab.masked_fill(~mask, -100)
        if cfg.text.roberta:  # masked LM: the label of a row is its own target
            shifted = lab
            pos_ids = _roberta_pos_ids(input_ids.to(torch.int64), cfg.text.pad_id).reshape(-1)
        else:
            shifted = torch.full_like(lab, -100)
            shifted[:, :-1] = lab[:, 1:]  # ForCausalLMLoss: pad(labels, (0,1)) then [..., 1:]
            if restart is not None:  # per document: its last token does not predict the next's first
                shifted[:, :-1].masked_fill_(restart[:, 1:], -100)
        shifted = shifted.reshape(-1)
        if mask is not None:  # drop the pads: everything below is over the T valid tokens
            sel = mask.reshape(-1)
            ids, shifted = ids[sel], shifted[sel]
            if cfg.text.roberta:
                pos_ids = pos_ids[sel]
        if cfg.text.roberta:
            self.pos_ids = _to(pos_ids, device, torch.int64)
        idn = ids.numpy()
        if idn.size and (idn.min() < 0 or idn.max() >= cfg.text.vocab):
            raise ValueError(f"token ids must lie in [0, {cfg.text.vocab})")
        keep = (shifted != -100).numpy()
        _check_labels(shifted.numpy()[keep], cfg.text.n_vocab)
        self.num_items = int(keep.sum())
        self.ids = _to(ids, device, torch.int64)
        self.labels = _to(shifted, device, torch.int64)
        # loss-row compaction (mmpt_gather_rows_bf16): the lm_head / CE run over the rows
        # whose label is not ignored — for LLaVA batches the image-token rows (their logits
        # are never consumed; their gradient is exactly zero), e.g. 511 of 707 rows for
        # ViT-B/16 + 511 text tokens.  Text-only batches keep every row but the last.
        self.loss_rows = self.loss_map = None
        self.loss_labels = self.labels
        if self.num_items < 0.95 * keep.size:
            idx = np.flatnonzero(keep)
            lmap = np.full(keep.size, -1, np.int32)
            lmap[idx] = np.arange(idx.size, dtype=np.int32)
            self.loss_rows = _to(torch.from_numpy(idx.astype(np.int32)), device, torch.int32)
            self.loss_labels = _to(shifted[torch.from_numpy(idx)], device, torch.int64)
            self.loss_map = _to(torch.from_numpy(lmap), device, torch.int32)
        self.img_map = None
        if cfg.multimodal:
            mask = idn == cfg.image_token_id
            n_img = int(mask.sum())
            expect = self.B * cfg.vision.num_patches
            if n_img != expect:  # tf:modeling_llava.py get_placeholder_mask raises likewise
                raise ValueError(f"image tokens {n_img} != features {expect}")
            imap = np.where(mask, np.cumsum(mask) - 1, -1).astype(np.int32)
            self.img_map = _to(torch.from_numpy(imap), device, torch.int32)

    def _from_device(self, cfg, input_ids, labels, device, mask=None, restart=None):
        self.ids = input_ids.to(device, torch.int64).contiguous().view(-1)
        sel = None
        if mask is not None:
            mask = mask.to(device)
            sel = mask.reshape(-1)
            self.ids = self.ids[sel].contiguous()
        # the embedding kernels index the table without bounds checks: validate here (the
        # path synchronises for the counts below anyway)
        if self.ids.numel():
            lo_hi = torch.stack((self.ids.min(), self.ids.max())).tolist()
            if lo_hi[0] < 0 or lo_hi[1] >= cfg.text.vocab:
                raise ValueError(f"token ids must lie in [0, {cfg.text.vocab})")
        lab = labels.to(device, torch.int64)
        if mask is not None:
            lab = lab.masked_fill(~mask, -100)
        if cfg.text.roberta:
            shifted = lab
            pos_ids = _roberta_pos_ids(input_ids.to(device, torch.int64), cfg.text.pad_id)
            pos_ids = pos_ids.reshape(-1)
            self.pos_ids = (pos_ids if sel is None else pos_ids[sel]).contiguous()
        else:
            shifted = torch.full_like(lab, -100)
            shifted[:, :-1] = lab[:, 1:]
            if restart is not None:
                shifted[:, :-1].masked_fill_(restart.to(device)[:, 1:], -100)
        self.labels = shifted.contiguous().view(-1)
        if sel is not None:
            self.labels = self.labels[sel].contiguous()
        keep = self.labels != -100
        self.num_items = int(keep.sum().item())
        if self.num_items:
            kept = self.labels[keep]
            _check_labels(torch.stack((kept.min(), kept.max())).cpu().numpy(), cfg.text.n_vocab)
        self.loss_rows = self.loss_map = None
        self.loss_labels = self.labels
        if self.num_items < 0.95 * self.labels.numel():
            idx = torch.nonzero(keep).view(-1)
            self.loss_rows = idx.to(torch.int32).contiguous()
            self.loss_labels = self.labels[idx].contiguous()
            self.loss_map = torch.full_like(self.labels, -1, dtype=torch.int32)
            self.loss_map[idx] = torch.arange(idx.numel(), device=self.labels.device,
                                              dtype=torch.int32)
        self.img_map = None
        if cfg.multimodal:
            mask = self.ids == cfg.image_token_id
            n_img = int(mask.sum().item())
            expect = self.B * cfg.vision.num_patches
            if n_img != expect:
                raise ValueError(f"image tokens {n_img} != features {expect}")
            self.img_map = torch.where(mask, mask.cumsum(0) - 1, -1).to(torch.int32).contiguous()

    def _segments(self, cfg: ModelConfig, device, keys=None, vocab=None) -> tuple:
        """Index bookkeeping for the deterministic embedding backward: the
        text rows stably sorted by token id, one segment per distinct id — built on the
        device by `mmpt_embed_segments` (seg_id, seg_off, perm, nseg, bad), the count left in
        HBM.  (A CPU `device` — host-logic tests only, the engine cannot run there — uses
        the numpy restatement `sort_segments`.)"""
        skip = cfg.image_token_id if cfg.multimodal else -1
        if cfg.text.roberta:  # padding_idx of both tables: no gradient from the gather
            skip = cfg.text.pad_id
        keys = self.ids if keys is None else keys  # (the position table: keyed by position id)
        vocab = cfg.text.vocab if vocab is None else vocab
        if device.type != "cuda":
            ids = keys.to("cpu", torch.int64).numpy()
            rows = np.arange(ids.size) if skip < 0 else np.flatnonzero(ids != skip)
            return tuple(torch.from_numpy(a) for a in sort_segments(ids, rows))
        return K.embed_segments(keys, vocab, skip)

    @property
    def tokens(self) -> int:
        """Token rows the step computes over (the valid tokens of a padded batch)."""
        return self.T


def _roberta_pos_ids(ids: torch.Tensor, pad_id: int) -> torch.Tensor:
    """tf:models/roberta/modeling_roberta.py create_position_ids_from_input_ids over [B, S] ids."""
    m = (ids != pad_id).to(torch.int64)
    return torch.cumsum(m, dim=1) * m + pad_id


def _check_labels(kept: np.ndarray, vocab_valid: int) -> None:
    """Labels other than -100 must index a real vocabulary row (torch's nll_loss asserts on
    the device; the cross-entropy kernel would report NaN for the row)."""
    if kept.size and (kept.min() < 0 or kept.max() >= vocab_valid):
        raise ValueError(f"labels must be -100 or lie in [0, {vocab_valid})")


def _dp_rank() -> int:
    import torch.distributed as dist

    return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0


def _to(t: torch.Tensor, device: torch.device, dtype) -> torch.Tensor:
    """Asynchronous host-to-device staging (pinned when the loader pinned it)."""
    t = t.to(dtype).contiguous()
    if device.type == "cuda" and t.device.type == "cpu":
        return t.to(device, non_blocking=t.is_pinned())
    return t.to(device)


def _drop_geometry(vl: Batch | None, B: int, S: int) -> dict:
    """The geometry keywords of K.attention_drop_fwd / _bwd: dense, or varlen over the batch vl."""
    if vl is None:
        return dict(batch=B, seq=S)
    return dict(lens=vl.lens, cu_seqlens=vl.cu_seqlens, max_seq=S)


class Engine:
    def __init__(self, cfg: ModelConfig, store: ParamStore, max_seq: int = 4096):
        self.cfg = cfg
        self.s = store
        self.dev = store.device
        t = cfg.text
        self.cos = self.sin = None  # a vision-only classifier has no rope
        if t is not None and not t.roberta and not t.mamba:  # (RoBERTa: learned positions)
            if t.llama:
                cos, sin = rope_tables_llama3(t.head_dim, t.rope_theta, t.rope_scaling, max_seq)
            else:
                cos, sin = rope_tables(t.hidden, t.heads, t.rotary_pct, t.rope_theta, max_seq)
            self.cos = cos.to(self.dev)
            self.sin = sin.to(self.dev)
        # the family's whole-model (forward, backward), and for the causal LMs the layer pair
        if cfg.convnext is not None:
            self._family = (self._convnext_forward, self._convnext_backward)
        elif cfg.classifier:
            self._family = (self._cls_forward, self._cls_backward)
        elif t.roberta:
            self._family = (self._roberta_forward, self._roberta_backward)
        else:
            self._family = (self._causal_forward, self._causal_backward)
            self._layer = (self._llama_layer_fwd, self._llama_layer_bwd) if t.llama else \
                (self._mamba_layer_fwd, self._mamba_layer_bwd) if t.mamba else \
                (self._text_layer_fwd, self._text_layer_bwd)
        # the qkv layouts of the text layers and of the ViT layers (_attention_fwd / _bwd)
        self._attn_t = self._attn_v = None
        if t is not None and not t.mamba:
            self._attn_t = AttnLayout.gqa(t) if t.llama else AttnLayout.planar(t) if t.roberta \
                else AttnLayout.neox(t)
        if cfg.multimodal:
            self._attn_v = AttnLayout.planar(cfg.vision)
        self.cache: dict = {}
        # activation checkpointing (HF gradient_checkpointing, src/train.py:112 →
        # TrainingClass.gradient_checkpointing): keep only each layer's input residual
        # stream in the forward and recompute the layer's forward right before its
        # backward (the recompute is not counted as model FLOPs, as in the reference)
        self.checkpointing = False
        # label smoothing of the loss (TrainingArguments.label_smoothing_factor, HF's
        # LabelSmoother): every cross entropy below, training and forward-only, takes it
        self.label_smoothing = 0.0
        # NEFTune (TrainingArguments.neftune_noise_alpha; HF's neftune_post_forward_hook on the
        # input embedding): None = off, else U(-m, m) noise on the token-embedding rows with
        # m = alpha / sqrt(Batch.S_in * hidden), drawn inside the gather kernels from
        # (dropout_seed, dropout_site(micro-step, rank, unit 0, k 4)) and never stored.  It
        # follows the hidden-dropout switch: on while dropout_enabled, off in eval
        self.neftune_alpha: float | None = None
        self._noise = None  # the K.EmbedNoise of the micro-step in flight
        # ZeRO-3 parameter residency (zero3.Zero3Residency): gathers a unit's weights
        # before use and reduce-scatters its gradients after its backward
        self.units = None
        # weight-gradient GEMMs on a second stream (see _dw)
        # (round 1 with gemm256: slower; round 5 with the persistent gemm4p: +0.6% at the bench
        # batch, +1.4% at 32 samples per rank — profiles/r05/dw_stream/)
        self.dw_stream = os.environ.get("MMPT_DW_STREAM", "1") == "1"
        # layers of weight-gradient work the side stream may run behind the compute stream
        self.dw_depth = max(1, int(os.environ.get("MMPT_DW_DEPTH", "1")))
        # bias gradients summed by the weight-gradient GEMM itself (K.gemm_wgrad_colsum) where
        # it takes the shape; MMPT_WGRAD_COLSUM=0: a separate column-sum pass (A/B)
        self.wgrad_colsum = os.environ.get("MMPT_WGRAD_COLSUM", "1") != "0"
        self._side = None
        self._pending: list = []
        self._fences: list = []
        # gradient-ready hook: called with a flat-buffer range [lo, hi) once every
        # gradient in it is final for this micro-batch (DDP overlap, distributed.GradSync)
        self.grad_ready_hook = None
        # every weight whose input gradient is needed gets a transposed bf16 shadow
        tied = t is not None and t.tie_embeddings
        self.head = "cls_head" if t is None else "text.embed" if tied else "text.lm_head"
        # LLaVA-pretrain freeze (src/models/llava.py:49-52): no weight gradients for the
        # tower / language model, no backward through the tower at all
        self.frozen = cfg.freeze_tower_and_llm
        store.transposed = [n for n in store.shapes if len(store.shapes[n]) == 2 and
                            n not in ("vision.patch.weight", "text.embed", "vision.pos",
                                      "text.pos_embed", "text.type_embed",
                                      "convnext.stem.weight") and
                            not n.endswith((".dw.weight", ".conv.weight", ".A_log"))]
        if tied:  # the tied lm_head's input gradient reads E^T
            store.transposed.append("text.embed")
        if self.frozen and not t.llama:
            raise NotImplementedError("freeze_tower_and_llm is the llava-pretrain (Llama) recipe")
        # hidden dropout (cfg.text / cfg.vision .hidden_dropout; a frozen tower has none).  The
        # masks are functions of (dropout_seed, dropout_site(micro-step, rank, unit, k)) and are
        # never stored: the micro-step counter advances once per forward(need_grad=True) and is
        # held for that step's backward and checkpoint recompute; accumulation micro-steps and
        # data-parallel ranks draw other masks.  dropout_enabled = False is eval(): the p = 0 path
        self.dropout_seed = 0
        self.dropout_enabled = True
        self.dropout_step = 0
        self.rank = _dp_rank()
        for layers in (t.layers if t is not None else 0,
                       cfg.vision.used_layers if cfg.multimodal else 0):
            if layers >= VISION_UNIT:
                raise ValueError(f"{layers} layers: dropout_site numbers at most {VISION_UNIT - 1}")
        self._pt = self._pv = 0.0  # the probabilities of the micro-step in flight
        self._pat = self._pav = 0.0  # ... of the attention-probability dropout (text, vision)
        # ConvNeXt stochastic depth (cfg.convnext.drop_path_rate): the per-block rates of the
        # micro-step in flight (None: the dense path) and its blocks' kept samples
        self._pdp = None
        self._kept: dict = {}
        if cfg.convnext is not None and sum(cfg.convnext.depths) >= VISION_UNIT:
            raise ValueError(f"{sum(cfg.convnext.depths)} blocks: dropout_site numbers at most "
                             f"{VISION_UNIT - 1}")
        self._dstep = 0
        if store.device.type == "cuda":
            store.refresh_transposed()

    def reset(self) -> None:
        """Drop every per-micro-batch state after a failed forward/backward (e.g. a
        torch.cuda.OutOfMemoryError caught by find_max_mbs_pow2 / the sweep's halving
        loop): the activation cache (incl. the logits), side-stream operands and fences,
        and the ZeRO-3 residency windows, so the retry starts from a clean engine and the
        caching allocator can release the failed micro-batch's memory."""
        if self._side is not None:
            self._side.synchronize()
        self.cache.clear()
        self._pending, self._fences = [], []
        self._recomputing = False
        if self.units is not None:
            self.units.reset()

    # -------------------------------------------------------------- helpers
    _recomputing = False

    def _restore(self, key, layer_fwd, i, B, S):
        """Activation checkpointing: re-run layer i's forward from its saved input."""
        ent = self.cache.get(key)
        if ent is None or ent[0] != "ckpt":
            return
        self._recomputing = True
        try:
            layer_fwd(i, ent[1], B, S)
        finally:
            self._recomputing = False

    def _unit_fwd(self, unit: str) -> None:
        if self.units is not None:
            self.units.forward(unit)

    def _unit_bwd(self, unit: str) -> None:
        if self.units is not None:
            self.units.backward(unit)

    def _unit_done(self, unit: str) -> None:
        if self.units is not None:
            self.units.backward_done(unit)

    # fp32 units (ZeRO-2/3 with DeepSpeed's persistence threshold: the token / position
    # embeddings partitioned, zero3.Zero3Store): gathered before their forward read, their
    # gradient window opened before and reduce-scattered after their backward
    def _is_f32_unit(self, name: str) -> bool:
        return self.units is not None and name in getattr(self.s, "fp32_units", ())

    def _f32_fwd(self, name: str) -> None:
        if self._is_f32_unit(name):
            self.units.forward(name)

    def _f32_bwd(self, name: str) -> None:
        if self._is_f32_unit(name):
            self.units.backward(name)

    def _f32_done(self, name: str) -> None:
        if self._is_f32_unit(name):
            self.units.backward_done(name)

    def _grad_open(self, unit: str) -> None:
        if self.units is not None:
            self.units.open_grad(unit)

    def unit_order(self) -> list[str]:
        """Forward order of the ZeRO-3 partition units (the parameters outside the
        fp32-read region, grouped per layer / module)."""
        cfg = self.cfg
        f32 = getattr(self.s, "fp32_units", ())
        order = []
        if cfg.convnext is not None:  # one unit per ConvNextStage, the stem and the head
            return ["convnext.stem"] + [f"convnext.stages.{s}" for s in range(4)] + ["cls_head"]
        if cfg.multimodal:
            order += ["vision.patch"] + (["vision.pos"] if "vision.pos" in f32 else [])
            order += [f"vision.layers.{i}" for i in range(cfg.vision.used_layers)]
            if cfg.classifier:
                return order + ["cls_head"]
            order += ["proj"]
        order += (["text.embed"] if "text.embed" in f32 else [])
        order += [f"text.layers.{i}" for i in range(cfg.text.layers)]
        if not cfg.text.tie_embeddings:
            order.append("text.lm_head")
        if cfg.text.roberta:
            order.append("text.mlm")
        return order

    def _ready(self, prefixes):
        """Announce that the grads of every parameter whose name starts with one of
        `prefixes` are final, as maximal contiguous runs of the flat buffer."""
        if self.grad_ready_hook is None:
            return
        spans = sorted((o, o + self.s.g(n).numel()) for n, o in self.s.offsets.items()
                       if n.startswith(prefixes))
        runs: list[list[int]] = []
        for lo, hi in spans:
            if runs and lo - runs[-1][1] < 64:  # only alignment padding in between
                runs[-1][1] = hi
            else:
                runs.append([lo, hi])
        side = self._side_stream()
        if side is None:
            for lo, hi in runs:
                self.grad_ready_hook(lo, hi)
            return
        # the collective must follow this group's weight grads (side stream) and its
        # LayerNorm / bias grads (compute stream): issue it from the side stream after
        # that stream has caught up with the compute stream
        side.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(side):
            for lo, hi in runs:
                self.grad_ready_hook(lo, hi)

    def _e(self, *shape, dtype=BF16):
        return torch.empty(*shape, dtype=dtype, device=self.dev)

    def _wn(self, name):
        """parameter name of a Linear's weight (the lm_head / tied embedding have no suffix)"""
        return name if name in self.s.shapes else name + ".weight"

    def _gw(self, name):
        """gradient tensor of a weight, or None when it is frozen (freeze_tower_and_llm)"""
        wn = self._wn(name)
        return self.s.g(wn) if self.cfg.trainable(wn) else None

    def _linear(self, x, name, out=None, bias=True, epi=K.EPI_BF16, aux=None, out2=None):
        W = self.s.w(self._wn(name))
        if out is None:
            out = self._e(x.shape[0], W.shape[0], dtype=F32 if epi == K.EPI_F32_RESID else BF16)
        b = self.s.w(name + ".bias") if bias else None
        K.gemm(x, W, out, epilogue=epi, bias=b, aux=aux, out2=out2)
        return out

    def _dx(self, dy, name):
        Wt = self.s.wt(self._wn(name))
        out = self._e(dy.shape[0], Wt.shape[0])
        K.gemm(dy, Wt, out)  # dX = dY·W = dY·(W^T)^T, both operands K-contiguous
        return out

    def _dx_dgelu(self, dy, name, pre, bias_of=None, quick=False):
        """dpre = bf16(dY·W) * gelu'(pre) (quick: CLIP's quick-GELU); with bias_of, that
        layer's bias gradient Σ_rows dpre is produced by the same GEMM (column sums in the
        epilogue)."""
        Wt = self.s.wt(name + ".weight")
        out = self._e(dy.shape[0], Wt.shape[0])
        if bias_of is None:
            K.gemm(dy, Wt, out, epilogue=K.EPI_BF16_DQGELU if quick else K.EPI_BF16_DGELU,
                   aux=pre)
        else:
            K.gemm_dgelu_colsum(dy, Wt, out, pre, self.s.g(bias_of + ".bias"), quick=quick)
        return out

    def _dw(self, dy, x, name, bias=True, bias2=None):
        """Weight (and bias) gradient.  With the weight-gradient stream enabled the GEMM
        runs there, concurrently with the input-gradient chain on the compute stream
        (it fills the CUs left idle by the other kernels' last tile waves); every gradient
        element is still written by exactly one stream, in micro-batch order."""
        if not self.cfg.trainable(self._wn(name)):
            return  # frozen: no weight (or bias) gradient
        G = self.s.g(self._wn(name))
        side = self._side_stream()
        if side is None:
            self._wgrad(dy, x, G, name, bias, bias2)
            return
        side.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(side):
            self._wgrad(dy, x, G, name, bias, bias2)
        # keep the operands alive until the compute stream is ordered after this GEMM
        # (_side_fence): freeing them earlier would let the caching allocator hand their
        # memory to a compute-stream kernel while the side stream still reads it.
        # (record_stream would instead defer every reuse to GPU progress, and with the
        # host far ahead of the GPU the allocator would grow until it thrashes.)
        self._pending.extend((dy, x))

    def _wgrad(self, dy, x, G, name, bias, bias2):
        """G += dyᵀ·x and, with `bias`, name.bias (and bias2.bias) += bf16(Σ_rows dy): one
        GEMM pass when the fused form takes the shape, else the GEMM then a column sum."""
        if bias:
            db = self.s.g(name + ".bias")
            db2 = None if bias2 is None else self.s.g(bias2 + ".bias")
            if self.wgrad_colsum and K.gemm_wgrad_colsum(dy, x, G, db, db2):
                return
        K.gemm(dy, x, G, layout_a=K.K_ROWS, layout_b=K.K_ROWS, epilogue=K.EPI_F32_ACC)
        if bias:
            K.colsum(dy, db, accumulate=True, dbias2=db2)

    def _side_stream(self):
        """The weight-gradient stream (None: everything on the compute stream).  A residency
        hook may veto it (`grads_on_compute_stream`); ZeRO-2/3 (zero3.Zero3Sync) takes it since
        round 5 — its per-unit reduce waits for this stream."""
        if (not self.dw_stream or self.dev.type != "cuda" or
                getattr(self.units, "grads_on_compute_stream", False)):
            return None
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.dev)
        # ZeRO-2/3: its gradient hooks wait for this stream — handed over on every call, so a
        # residency object installed after the stream was created gets it too
        if getattr(self.units, "side", 0) is None:
            self.units.side = self._side
        return self._side

    def _side_fence(self) -> None:
        """Called as each layer's backward starts: the compute stream waits for the side
        stream's work of two layers up, then that work's operands are released — one
        layer of weight-gradient GEMMs stays in flight beside the input-gradient chain."""
        if self._side is None:
            return
        ev = torch.cuda.Event()
        ev.record(self._side)
        self._fences.append((ev, self._pending))
        self._pending = []
        while len(self._fences) > self.dw_depth:
            ev0, _ = self._fences.pop(0)
            torch.cuda.current_stream(self.dev).wait_event(ev0)

    def _join_side(self) -> None:
        if self._side is not None:
            torch.cuda.current_stream(self.dev).wait_stream(self._side)
            self._fences, self._pending = [], []

    # -------------------------------------------------------------- the step frame
    # What every family's forward and backward share.  Padded and packed batches
    # (Batch.cu_seqlens set): the text layers run over the T valid tokens.  Every buffer is sized
    # by the residual stream's row count, `S` is the longest sequence (Batch.max_len: the varlen
    # kernels' max_seq and the lse stride), attention, the Mamba conv and the scan take their
    # varlen entries and the rope reads each token's position from Batch.pos.  _vl is the batch
    # of the forward / backward in flight, or None on the dense path (image batches always).
    _vl = None

    def _begin(self, batch: Batch, need_grad: bool) -> None:
        """The forward's prologue: the varlen state, the staged batch handed to the compute
        stream, the residency region, the micro-step's dropout state (the image classifiers
        draw no embedding noise)."""
        self._vl = batch if batch.cu_seqlens is not None else None
        if self.dev.type == "cuda":
            batch.use(torch.cuda.current_stream(self.dev))
        region = getattr(self.units, "region", None)
        if region is not None:  # an overlapped optimizer update of the fp32-read region
            region()
        if self.cos is not None and batch.max_len > self.cos.shape[0]:
            raise ValueError(f"sequence {batch.max_len} longer than the rope table "
                             f"{self.cos.shape[0]}")
        self._drop_begin(need_grad, None if self.cfg.classifier else batch)

    def _loss(self, logits, batch: Batch, vocab_valid: int, grad_scale: float,
              need_grad: bool) -> torch.Tensor:
        """Σ_rows CE over the bf16 logits (device fp32 [1]), the forward's last act.  With
        need_grad the logits become dlogits in place and the cache entries the family has set
        stay for the backward; without, nothing of the step is kept."""
        loss_rows = self._e(logits.shape[0], dtype=F32)
        K.cross_entropy(logits, batch.loss_labels, -100, grad_scale, loss_rows,
                        logits if need_grad else None, vocab_valid=vocab_valid,
                        label_smoothing=self.label_smoothing)
        loss = self._e(1, dtype=F32)
        K.sum_f32(loss_rows, loss)
        if not need_grad:
            self.cache.clear()
        return loss

    def _begin_backward(self, batch: Batch, scale: torch.Tensor | None) -> tuple:
        """The backward's prologue: the head's cache entry, its last element the dlogits
        (times `scale`)."""
        self._vl = batch if batch.cu_seqlens is not None else None
        head = self.cache.pop("head")
        if scale is not None:
            head[-1].mul_(scale.to(torch.float32))
        return head

    def _finish(self) -> None:
        """The backward's epilogue."""
        self._join_side()
        self.cache.clear()

    def _scored_rows(self, y, batch: Batch):
        """Loss-row compaction: the rows of y that carry a label (y itself when most do)."""
        if batch.loss_rows is None:
            return y
        yv = self._e(batch.loss_rows.numel(), y.shape[1])
        K.gather_rows(y, batch.loss_rows, yv)
        return yv

    def _all_rows(self, dy, batch: Batch):
        """Backward of _scored_rows: back to every row, zero where the label is ignored."""
        if batch.loss_map is None:
            return dy
        out = self._e(batch.T, dy.shape[1])
        K.expand_rows(dy, batch.loss_map, out)
        return out

    # -------------------------------------------------------------- attention
    def _attention_fwd(self, lay: AttnLayout, unit: int, p: float, qkv, B, S, a, lse,
                       vl: Batch | None = None) -> None:
        """Attention of every transformer layer: with probability dropout p at site k = 2 of
        `unit` (the checkpoint recompute redraws the same mask), varlen over the batch vl, GQA or
        plain.  The vision tower passes no vl: images are dense whatever the text batch is."""
        H, Hk, D, hs, koff, voff, causal = lay
        sc = D ** -0.5
        if p > 0:
            K.attention_drop_fwd(qkv, H, Hk, D, hs, koff, voff, causal, sc, a, lse, p,
                                 self.dropout_seed, self._site(unit, 2),
                                 **_drop_geometry(vl, B, S))
        elif vl is not None:
            K.attention_varlen_fwd(qkv, vl.lens, vl.cu_seqlens, H, Hk, D, hs, koff, voff, causal,
                                   sc, a, lse, max_seq=S)
        elif Hk != H:
            K.attention_gqa_fwd(qkv, B, S, H, Hk, D, koff, voff, causal, sc, a, lse)
        else:
            K.attention_fwd(qkv, B, S, H, D, hs, koff, causal, sc, a, lse)

    def _attention_bwd(self, lay: AttnLayout, unit: int, p: float, qkv, B, S, a, da, lse, dqkv,
                       rot_dims: int = 0, vl: Batch | None = None) -> None:
        """Backward of _attention_fwd (same site).  rot_dims > 0 (GPTNeoX): also the rope backward
        of dqkv's q and k parts — in the dK / dQ epilogues of the dense entry, a pass of its own
        after the dropout and varlen entries (ring dK/dV + recomputing dQ), which fuse none."""
        H, Hk, D, hs, koff, voff, causal = lay
        sc = D ** -0.5
        if p > 0:
            K.attention_drop_bwd(qkv, H, Hk, D, hs, koff, voff, causal, sc, a, da, lse, dqkv, p,
                                 self.dropout_seed, self._site(unit, 2),
                                 **_drop_geometry(vl, B, S))
        elif vl is not None:
            K.attention_varlen_bwd(qkv, vl.lens, vl.cu_seqlens, H, Hk, D, hs, koff, voff, causal,
                                   sc, a, da, lse, dqkv, max_seq=S)
        elif rot_dims > 0:
            K.attention_bwd_rope(qkv, B, S, H, D, hs, koff, causal, sc, a, da, lse, dqkv,
                                 rot_dims, self.cos, self.sin)
            return
        elif Hk != H:
            K.attention_gqa_bwd(qkv, B, S, H, Hk, D, koff, voff, causal, sc, a, da, lse, dqkv)
        else:
            K.attention_bwd(qkv, B, S, H, D, hs, koff, causal, sc, a, da, lse, dqkv)
        if rot_dims > 0:
            self._rope(dqkv, S, H, D, rot_dims, hs, koff, inverse=True)

    def _rope(self, qkv, S, heads, D, rot, head_stride, part_stride, inverse=False, parts=2,
              offset=0):
        K.rope_inplace(qkv, S, heads, D, rot, head_stride, part_stride, self.cos, self.sin,
                       inverse=inverse, parts=parts, offset=offset,
                       pos=None if self._vl is None else self._vl.pos)

    # -------------------------------------------------------------- hidden dropout
    def _site(self, unit: int, k: int) -> int:
        return dropout_site(self._dstep, self.rank, unit, k)

    def _drop_begin(self, need_grad: bool, batch: Batch | None = None) -> None:
        """Fix the micro-step's dropout state (probabilities, mask counter, and with `batch` the
        embedding noise's magnitude and site) for the forward, its backward and any recompute.  A
        forward without gradients previews the next step's masks and leaves the counter alone."""
        on = self.dropout_enabled
        self._pt = self.cfg.text.hidden_dropout if on and self.cfg.text is not None else 0.0
        self._pv = self.cfg.vision.hidden_dropout if on and self.cfg.multimodal and \
            not self.frozen else 0.0
        self._pat = self.cfg.text.attn_dropout if on and self.cfg.text is not None else 0.0
        self._pav = self.cfg.vision.attention_dropout if on and self.cfg.multimodal and \
            not self.frozen else 0.0
        self._dstep = self.dropout_step
        # stochastic depth is training only: a forward without gradients runs every block densely
        cn = self.cfg.convnext
        self._pdp = cn.drop_path_rates() if on and need_grad and cn is not None and \
            cn.drop_path_rate > 0 else None
        self._kept = {}
        self._noise = None
        if on and batch is not None and self.neftune_alpha:
            self._noise = K.EmbedNoise(
                K.embed_noise_mag(self.neftune_alpha, batch.S_in, self.cfg.text.hidden),
                self.dropout_seed, self._site(0, 4))
        if need_grad and (max(self._pt, self._pv, self._pat, self._pav) > 0 or
                          self._pdp is not None or self._noise is not None):
            self.dropout_step += 1

    def _drop_grad(self, d, p, unit, k, bias, out=None):
        """A dropped branch's gradient drop(d) (same site as the forward; in place unless `out`)
        and its Linear's bias gradient: the column sum of the masked gradient."""
        out = d if out is None else out
        K.dropout_bf16(d, out, p, self.dropout_seed, self._site(unit, k))
        K.colsum(out, self.s.g(bias), accumulate=True)
        return out

    # -------------------------------------------------------------- text layers
    def _text_layer_fwd(self, i, x, B, S):
        t = self.cfg.text
        T, h, H, D = x.shape[0], t.hidden, t.heads, t.head_dim
        p = f"text.layers.{i}."
        y1, y2 = self._e(T, h), self._e(T, h)
        mean, rstd = self._e(T, dtype=F32), self._e(T, dtype=F32)
        K.layernorm_fwd(x, self.s.p(p + "ln1.weight"), self.s.p(p + "ln1.bias"), t.eps, y1, mean,
                        rstd, self.s.p(p + "ln2.weight"), self.s.p(p + "ln2.bias"), y2)
        qkv = self._linear(y1, p + "qkv")
        if t.rot_dims > 0:
            self._rope(qkv, S, H, D, t.rot_dims, 3 * D, D)
        a = self._e(T, h)
        lse = self._e(B * H * S, dtype=F32)
        self._attention_fwd(self._attn_t, 1 + i, self._pat, qkv, B, S, a, lse, vl=self._vl)
        ap = self._linear(a, p + "dense")
        pre, act = self._e(T, t.ffn), self._e(T, t.ffn)
        self._linear(y2, p + "fc1", out=pre, epi=K.EPI_BF16_GELU, out2=act)
        xn = self._e(T, h, dtype=F32)
        # h' = (mlp + attn) [bf16 add] + h [fp32]   (tf:modeling_gpt_neox.py:271-274)
        if self._pt > 0:  # h' = bf16(drop(mlp) + drop(attn)) + h: post_mlp / post_attention_dropout
            mlp = self._linear(act, p + "fc2")
            K.dropout_add_f32(ap, self._site(1 + i, 0), x, xn, self._pt, self.dropout_seed,
                              y2=mlp, site_y2=self._site(1 + i, 1))
        else:
            self._linear(act, p + "fc2", out=xn, epi=K.EPI_F32_RESID, aux=ap, out2=x)
        if self.checkpointing and not self._recomputing:
            self.cache[("t", i)] = ("ckpt", x)
        else:
            self.cache[("t", i)] = (x, mean, rstd, y1, y2, qkv, a, lse, pre, act)
        return xn

    def _resid_grad_targets(self, i, T):
        """bf16 copy + bias-gradient targets for text layer i's residual-stream gradient (T
        rows): d(fc2.bias) == d(dense.bias) == Σ bf16(dh) under the parallel residual."""
        if i < 0:
            return {}
        p = f"text.layers.{i}."
        self._grad_open(f"text.layers.{i}")
        if self._pt > 0:  # the two biases then see differently masked gradients (_drop_grad)
            return dict(dx_bf16=self._e(T, self.cfg.text.hidden))
        return dict(dx_bf16=self._e(T, self.cfg.text.hidden), dsum=self.s.g(p + "fc2.bias"),
                    dsum2=self.s.g(p + "dense.bias"))

    def _text_layer_bwd(self, i, dxn, ds, B, S):
        """dxn: fp32 gradient of layer i's output; ds = bf16(dxn), the grad of the bf16
        (mlp + attn) sum, produced (with the fc2/dense bias gradients) by the layer
        above's fused LayerNorm backward."""
        t = self.cfg.text
        T, h = dxn.shape[0], t.hidden
        p = f"text.layers.{i}."
        self._side_fence()
        self._unit_bwd(f"text.layers.{i}")
        self._restore(("t", i), self._text_layer_fwd, i, B, S)
        x, mean, rstd, y1, y2, qkv, a, lse, pre, act = self.cache.pop(("t", i))
        dsa = ds  # the gradients of the dense (attention) and fc2 (MLP) outputs
        if self._pt > 0:  # each branch: drop(bf16(d residual)) with the forward's site
            dsa = self._drop_grad(ds, self._pt, 1 + i, 0, p + "dense.bias", out=self._e(T, h))
            ds = self._drop_grad(ds, self._pt, 1 + i, 1, p + "fc2.bias")
        dpre = self._dx_dgelu(ds, p + "fc2", pre, bias_of=p + "fc1")
        self._dw(ds, act, p + "fc2", bias=False)
        dy2 = self._dx(dpre, p + "fc1")
        self._dw(dpre, y2, p + "fc1", bias=False)
        da = self._dx(dsa, p + "dense")
        self._dw(dsa, a, p + "dense", bias=False)
        dqkv = self._e(T, 3 * h)
        self._attention_bwd(self._attn_t, 1 + i, self._pat, qkv, B, S, a, da, lse, dqkv,
                            rot_dims=t.rot_dims, vl=self._vl)
        dy1 = self._dx(dqkv, p + "qkv")
        self._dw(dqkv, y1, p + "qkv")
        # dx = dxn + LN1'(dy1) + LN2'(dy2)  (in place over dxn), + bf16 copy for layer i-1
        nxt = self._resid_grad_targets(i - 1, T)
        K.layernorm_bwd(x, mean, rstd, dy1, self.s.p(p + "ln1.weight"), dxn,
                        self.s.g(p + "ln1.weight"), self.s.g(p + "ln1.bias"), dy2,
                        self.s.p(p + "ln2.weight"), self.s.g(p + "ln2.weight"),
                        self.s.g(p + "ln2.bias"), dresid=dxn, **nxt)
        self._unit_done(f"text.layers.{i}")
        return dxn, nxt.get("dx_bf16")

    # -------------------------------------------------------------- llama layers
    def _llama_layer_fwd(self, i, x, B, S):
        """LlamaDecoderLayer (tf:models/llama/modeling_llama.py:284-324) under autocast:
        h = x + bf16(o_proj(attn(RMS1 x)));  x' = h + bf16(down(bf16(silu(g)) * u)), with
        g|u = gate_up(RMS2 h) in one GEMM (blocked weight, SwiGLU epilogue), q/k/v in one
        GEMM, llama3 RoPE in place, GQA flash attention."""
        t = self.cfg.text
        T, h, H, Hk, D = x.shape[0], t.hidden, t.heads, t.n_kv, t.head_dim
        p = f"text.layers.{i}."
        y1, r1 = self._e(T, h), self._e(T, dtype=F32)
        K.rmsnorm_fwd(x, self.s.p(p + "ln1.weight"), t.eps, y1, r1)
        qkv = self._linear(y1, p + "qkv", bias=False)
        self._rope(qkv, S, H, D, D, D, 0, parts=1)
        self._rope(qkv, S, Hk, D, D, D, 0, parts=1, offset=H * D)
        a = self._e(T, h)
        lse = self._e(B * H * S, dtype=F32)
        self._attention_fwd(self._attn_t, 1 + i, self._pat, qkv, B, S, a, lse, vl=self._vl)
        h1 = self._linear(a, p + "dense", bias=False, epi=K.EPI_F32_RESID, out2=x)
        y2, r2 = self._e(T, h), self._e(T, dtype=F32)
        K.rmsnorm_fwd(h1, self.s.p(p + "ln2.weight"), t.eps, y2, r2)
        gu, act = self._e(T, 2 * t.ffn), self._e(T, t.ffn)
        self._linear(y2, p + "gate_up", out=gu, bias=False, epi=K.EPI_BF16_SWIGLU, out2=act)
        xn = self._linear(act, p + "down", bias=False, epi=K.EPI_F32_RESID, out2=h1)
        if self.checkpointing and not self._recomputing:
            self.cache[("t", i)] = ("ckpt", x)
        else:
            self.cache[("t", i)] = (x, r1, y1, qkv, a, lse, h1, r2, y2, gu, act)
        return xn

    def _llama_layer_bwd(self, i, dxn, ds, B, S):
        """dxn: fp32 gradient of layer i's output, ds = bf16(dxn) (the down_proj output's
        gradient).  Returns (dx, bf16(dx)) for layer i-1."""
        t = self.cfg.text
        T, h, H, Hk, D = dxn.shape[0], t.hidden, t.heads, t.n_kv, t.head_dim
        p = f"text.layers.{i}."
        self._side_fence()
        self._unit_bwd(f"text.layers.{i}")
        self._restore(("t", i), self._llama_layer_fwd, i, B, S)
        x, r1, y1, qkv, a, lse, h1, r2, y2, gu, act = self.cache.pop(("t", i))
        # d act = ds·W_down -> (d gate, d up) by the SwiGLU-backward epilogue
        dgu = self._e(T, 2 * t.ffn)
        K.gemm(ds, self.s.wt(p + "down.weight"), dgu, epilogue=K.EPI_BF16_DSWIGLU, aux=gu)
        self._dw(ds, act, p + "down", bias=False)
        dy2 = self._dx(dgu, p + "gate_up")
        self._dw(dgu, y2, p + "gate_up", bias=False)
        # dh1 = dxn + RMS2'(dy2) (in place); d1 = bf16(dh1), the o_proj output's gradient
        d1 = self._e(T, h)
        K.rmsnorm_bwd(h1, r2, dy2, self.s.p(p + "ln2.weight"), dxn, dw=self._gw(p + "ln2"),
                      dresid=dxn, dx_bf16=d1)
        da = self._dx(d1, p + "dense")
        self._dw(d1, a, p + "dense", bias=False)
        dqkv = self._e(T, t.qkv_dim)
        self._attention_bwd(self._attn_t, 1 + i, self._pat, qkv, B, S, a, da, lse, dqkv,
                            vl=self._vl)
        self._rope(dqkv, S, H, D, D, D, 0, inverse=True, parts=1)
        self._rope(dqkv, S, Hk, D, D, D, 0, inverse=True, parts=1, offset=H * D)
        dy1 = self._dx(dqkv, p + "qkv")
        self._dw(dqkv, y1, p + "qkv", bias=False)
        nxt = self._e(T, h) if i > 0 else None
        K.rmsnorm_bwd(x, r1, dy1, self.s.p(p + "ln1.weight"), dxn, dw=self._gw(p + "ln1"),
                      dresid=dxn, dx_bf16=nxt)
        self._unit_done(f"text.layers.{i}")
        return dxn, nxt

    # -------------------------------------------------------------- vision
    def _vit_layer_fwd(self, i, x, B, Sv):
        v = self.cfg.vision
        T, h, H = B * Sv, v.hidden, v.heads
        p = f"vision.layers.{i}."
        y1 = self._e(T, h)
        m1, r1 = self._e(T, dtype=F32), self._e(T, dtype=F32)
        K.layernorm_fwd(x, self.s.p(p + "ln1.weight"), self.s.p(p + "ln1.bias"), v.eps, y1, m1, r1)
        qkv = self._linear(y1, p + "qkv")
        a = self._e(T, h)
        lse = self._e(B * H * Sv, dtype=F32)
        pv, u = self._pv, VISION_UNIT + 1 + i
        self._attention_fwd(self._attn_v, u, self._pav, qkv, B, Sv, a, lse)
        if pv > 0:  # h1 = x + drop(o): ViTSelfOutput.dropout
            h1 = self._e(T, h, dtype=F32)
            K.dropout_add_f32(self._linear(a, p + "o"), self._site(u, 0), x, h1, pv,
                              self.dropout_seed)
        else:
            h1 = self._linear(a, p + "o", epi=K.EPI_F32_RESID, out2=x)
        y2 = self._e(T, h)
        m2, r2 = self._e(T, dtype=F32), self._e(T, dtype=F32)
        K.layernorm_fwd(h1, self.s.p(p + "ln2.weight"), self.s.p(p + "ln2.bias"), v.eps, y2, m2, r2)
        pre, act = self._e(T, v.ffn), self._e(T, v.ffn)
        self._linear(y2, p + "fc1", out=pre, out2=act,
                     epi=K.EPI_BF16_QGELU if v.act == "quick_gelu" else K.EPI_BF16_GELU)
        if pv > 0:  # x' = h1 + drop(fc2): ViTOutput.dropout
            xn = self._e(T, h, dtype=F32)
            K.dropout_add_f32(self._linear(act, p + "fc2"), self._site(u, 1), h1, xn, pv,
                              self.dropout_seed)
        else:
            xn = self._linear(act, p + "fc2", epi=K.EPI_F32_RESID, out2=h1)
        if self.frozen:
            pass  # frozen tower: no backward through it, nothing to keep
        elif self.checkpointing and not self._recomputing:
            self.cache[("v", i)] = ("ckpt", x)
        else:
            self.cache[("v", i)] = (x, m1, r1, y1, qkv, a, lse, h1, m2, r2, y2, pre, act)
        return xn

    def _vit_layer_bwd(self, i, dxn, d2, B, Sv):
        """d2 = bf16(dxn) with fc2.bias's gradient already accumulated (by the layer
        above's fused LN backward, or the caller for the top layer)."""
        v = self.cfg.vision
        T, h = B * Sv, v.hidden
        p = f"vision.layers.{i}."
        self._side_fence()
        self._unit_bwd(f"vision.layers.{i}")
        self._restore(("v", i), self._vit_layer_fwd, i, B, Sv)
        x, m1, r1, y1, qkv, a, lse, h1, m2, r2, y2, pre, act = self.cache.pop(("v", i))
        pv, u = self._pv, VISION_UNIT + 1 + i
        if pv > 0:  # d2 arrives unmasked and without fc2.bias's gradient
            d2 = self._drop_grad(d2, pv, u, 1, p + "fc2.bias")
        dpre = self._dx_dgelu(d2, p + "fc2", pre, bias_of=p + "fc1", quick=v.act == "quick_gelu")
        self._dw(d2, act, p + "fc2", bias=False)
        dy2 = self._dx(dpre, p + "fc1")
        self._dw(dpre, y2, p + "fc1", bias=False)
        # dh1 = dxn + LN2'(dy2)   (in place), d1 = bf16(dh1), d(o.bias) = Σ d1
        d1 = self._e(T, h)
        K.layernorm_bwd(h1, m2, r2, dy2, self.s.p(p + "ln2.weight"), dxn,
                        self.s.g(p + "ln2.weight"), self.s.g(p + "ln2.bias"), dresid=dxn,
                        dx_bf16=d1, dsum=None if pv > 0 else self.s.g(p + "o.bias"))
        if pv > 0:
            self._drop_grad(d1, pv, u, 0, p + "o.bias")
        da = self._dx(d1, p + "o")
        self._dw(d1, a, p + "o", bias=False)
        dqkv = self._e(T, 3 * h)
        self._attention_bwd(self._attn_v, u, self._pav, qkv, B, Sv, a, da, lse, dqkv)
        dy1 = self._dx(dqkv, p + "qkv")
        self._dw(dqkv, y1, p + "qkv")
        if i > 0:
            self._grad_open(f"vision.layers.{i - 1}")
        nxt = {} if i == 0 else dict(dx_bf16=self._e(T, h),
                                     dsum=self.s.g(f"vision.layers.{i - 1}.fc2.bias"))
        if pv > 0:
            nxt.pop("dsum", None)
        K.layernorm_bwd(x, m1, r1, dy1, self.s.p(p + "ln1.weight"), dxn,
                        self.s.g(p + "ln1.weight"), self.s.g(p + "ln1.bias"), dresid=dxn, **nxt)
        self._unit_done(f"vision.layers.{i}")
        return dxn, nxt.get("dx_bf16")

    def _encoder_fwd(self, pixels, B):
        """Embeddings + the used encoder layers: the fp32 residual stream [B·(patches+1), h]
        (what the projector path and the classification head both read), the im2col buffer
        and the pre-LN's saved tensors for the embedding backward."""
        v = self.cfg.vision
        npch, hv = v.num_patches, v.hidden
        cols = self._e(B * npch, v.patch_k)
        K.im2col(pixels, v.patch, cols)
        self._unit_fwd("vision.patch")
        po = self._linear(cols, "vision.patch", bias=v.patch_bias)
        h = self._e(B * (npch + 1), hv, dtype=F32)
        self._f32_fwd("vision.pos")
        K.vit_embed_fwd(B, npch, po, self.s.p("vision.cls"), self.s.p("vision.pos"), h)
        if self._pv > 0:  # ViTEmbeddings.dropout, after the position add
            K.dropout_f32(h, h, self._pv, self.dropout_seed, self._site(VISION_UNIT, 0))
        pre_ln = None
        if v.pre_ln:  # CLIP pre_layrnorm: fp32 in, fp32 residual stream out
            e = h
            h = self._e(B * (npch + 1), hv, dtype=F32)
            m0, r0 = self._e(B * (npch + 1), dtype=F32), self._e(B * (npch + 1), dtype=F32)
            K.layernorm_f32_fwd(e, self.s.p("vision.ln_pre.weight"), self.s.p("vision.ln_pre.bias"),
                                v.eps, h, m0, r0)
            pre_ln = (e, m0, r0)
        for i in range(v.used_layers):
            self._unit_fwd(f"vision.layers.{i}")
            h = self._vit_layer_fwd(i, h, B, npch + 1)
        return h, cols, pre_ln

    def _vision_fwd(self, pixels, B):
        v = self.cfg.vision
        npch, hv = v.num_patches, v.hidden
        h, cols, pre_ln = self._encoder_fwd(pixels, B)
        f = self._e(B * npch, hv)
        K.select_patches_fwd(B, npch, h, f)
        ht = self.cfg.text.hidden
        ppre, pact = self._e(B * npch, ht), self._e(B * npch, ht)
        self._unit_fwd("proj")
        self._linear(f, "proj.fc1", out=ppre, epi=K.EPI_BF16_GELU, out2=pact)
        img = self._linear(pact, "proj.fc2")
        self.cache["vis"] = (cols, f, ppre, pact, pre_ln)
        return img

    def _vision_bwd(self, dimg, B):
        v = self.cfg.vision
        npch, hv = v.num_patches, v.hidden
        cols, f, ppre, pact, pre_ln = self.cache.pop("vis")
        self._side_fence()
        self._unit_bwd("proj")
        dppre = self._dx_dgelu(dimg, "proj.fc2", ppre, bias_of="proj.fc1")
        self._dw(dimg, pact, "proj.fc2")
        if self.frozen:  # the tower is frozen: nothing below the projector needs a gradient
            self._dw(dppre, f, "proj.fc1", bias=False)
            self._unit_done("proj")
            return
        df = self._dx(dppre, "proj.fc1")
        self._dw(dppre, f, "proj.fc1", bias=False)
        self._unit_done("proj")
        dh = self._e(B * (npch + 1), hv, dtype=F32)
        K.select_patches_bwd(B, npch, df, dh, accumulate=False)
        top = v.used_layers - 1
        self._grad_open(f"vision.layers.{top}")
        d2 = self._e(B * (npch + 1), hv)
        K.cast_f32_bf16(dh, d2)
        if self._pv == 0:  # else the layer sums its masked gradient itself
            K.colsum(d2, self.s.g(f"vision.layers.{top}.fc2.bias"), accumulate=True)
        self._encoder_bwd(dh, d2, B, cols, pre_ln)

    def _encoder_bwd(self, dh, d2, B, cols, pre_ln):
        """Backward of _encoder_fwd from the top layer's output gradient: dh fp32, d2 = bf16(dh)
        (with the top layer's fc2.bias gradient already summed when vision dropout is 0)."""
        v = self.cfg.vision
        npch, hv = v.num_patches, v.hidden
        for i in reversed(range(v.used_layers)):
            dh, d2 = self._vit_layer_bwd(i, dh, d2, B, npch + 1)
        if pre_ln is not None:  # through pre_layrnorm (its γ/β grads accumulate)
            e, m0, r0 = pre_ln
            de = torch.empty_like(dh)
            K.layernorm_f32_bwd(e, m0, r0, dh, self.s.p("vision.ln_pre.weight"), de,
                                self.s.g("vision.ln_pre.weight"), self.s.g("vision.ln_pre.bias"))
            dh = de
        if self._pv > 0:
            K.dropout_f32(dh, dh, self._pv, self.dropout_seed, self._site(VISION_UNIT, 0))
        dpo = self._e(B * npch, hv)
        self._f32_bwd("vision.pos")
        K.vit_embed_bwd(B, npch, dh, self.s.g("vision.cls"), self.s.g("vision.pos"), dpo)
        self._f32_done("vision.pos")
        self._unit_bwd("vision.patch")
        self._dw(dpo, cols, "vision.patch", bias=v.patch_bias)
        self._unit_done("vision.patch")

    # -------------------------------------------------------------- classification head
    def _cls_forward(self, batch: Batch, grad_scale: float, need_grad: bool) -> torch.Tensor:
        """ViTForImageClassification (tf:models/vit/modeling_vit.py): encoder, vit.layernorm on
        the CLS rows (the only ones the head reads), classifier with its bias, Σ_images CE."""
        cfg, v = self.cfg, self.cfg.vision
        B, Sv = batch.B, v.num_patches + 1
        self._begin(batch, need_grad)
        h, cols, pre_ln = self._encoder_fwd(batch.pixels, B)
        y = self._e(B, v.hidden)
        m, r = self._e(B, dtype=F32), self._e(B, dtype=F32)
        K.cls_ln_fwd(h, B, Sv, self.s.p("vision.ln_post.weight"), self.s.p("vision.ln_post.bias"),
                     v.eps, y, m, r)
        self._unit_fwd("cls_head")
        logits = self._linear(y, "cls_head")
        self.cache["head"] = (h, m, r, y, logits)
        self.cache["vis"] = (cols, pre_ln)
        return self._loss(logits, batch, cfg.num_classes, grad_scale, need_grad)

    def _cls_backward(self, batch: Batch, scale: torch.Tensor | None) -> None:
        v = self.cfg.vision
        B, Sv = batch.B, v.num_patches + 1
        hL, m, r, y, dlogits = self._begin_backward(batch, scale)
        cols, pre_ln = self.cache.pop("vis")
        self._unit_bwd("cls_head")
        dy = self._dx(dlogits, "cls_head")
        self._dw(dlogits, y, "cls_head")  # + the classifier's bias gradient
        self._unit_done("cls_head")
        del dlogits
        # vit.layernorm's backward, the zero rows of the residual-stream gradient and its bf16
        # copy in one pass; without dropout also the top layer's fc2.bias gradient (the layer
        # sums its masked gradient itself otherwise)
        top = f"vision.layers.{v.used_layers - 1}"
        self._grad_open(top)
        dh, d2 = self._e(B * Sv, v.hidden, dtype=F32), self._e(B * Sv, v.hidden)
        K.cls_ln_bwd(hL, B, Sv, m, r, dy, self.s.p("vision.ln_post.weight"), dh, d2,
                     self.s.g("vision.ln_post.weight"), self.s.g("vision.ln_post.bias"),
                     dsum=None if self._pv > 0 else self.s.g(top + ".fc2.bias"))
        self._encoder_bwd(dh, d2, B, cols, pre_ln)
        self._ready(("vision.", "cls_head."))
        self._finish()

    # -------------------------------------------------------------- ConvNeXt
    # The residual stream x is fp32 [B·H·W, C], channels-last.  A block keeps (x, c, mean, rstd,
    # n, pre, act, y) for its backward; with activation checkpointing a STAGE keeps only its
    # input and is recomputed before its backward (the reference's
    # ConvNextEncoderWithCheckpointing wraps each ConvNextStage).  Stochastic depth
    # (drop_path_rate > 0, training): a block with drop probability > 0 runs over its kept samples
    # only (_cn_block_drop_fwd / _bwd) and additionally keeps their map and its probability.
    # _convnext_forward / _backward are the family's body inside the step frame.
    def _cn_f32_of_bf16(self, x, name):
        """f32(bf16(x·Wᵀ + b)): a conv output (bf16 under autocast) held exactly in the fp32
        stream — the residual epilogue over a zero residual."""
        W = self.s.w(name + ".weight")
        zero = torch.zeros(x.shape[0], W.shape[0], dtype=F32, device=self.dev)
        return self._linear(x, name, epi=K.EPI_F32_RESID, out2=zero)

    def _cn_kept(self, j, B):
        """Block j's kept samples under stochastic depth, decided on the host: the keep bits of
        site (micro-step, rank, VISION_UNIT + 1 + j, 3), elements 0 .. B-1.  The tables of every
        block of the micro-step are drawn on first use and go to the device in one copy; a
        recompute under activation checkpointing finds them again."""
        if not self._kept:
            js = [i for i, p in enumerate(self._pdp) if p > 0]
            idxs = kept_indices_of(B, [self._pdp[i] for i in js], self.dropout_seed,
                                   [self._site(VISION_UNIT + 1 + i, 3) for i in js])
            self._kept = dict(zip(js, K.kept_samples_of(B, idxs, self.dev)))
        return self._kept[j]

    def _cn_block_drop_fwd(self, p, x, B, side, j):
        """_cn_block_fwd over the kept samples of block j (drop probability > 0): the branch is
        computed for them alone, compactly; dropped planes of x are copied.  Nobody kept: the
        block is the identity and saves nothing."""
        kept, pj = self._cn_kept(j, B), self._pdp[j]
        if kept.Bk == 0:
            return x, None
        R, C = x.shape
        rps = side * side
        Rk = kept.Bk * rps
        c = self._e(Rk, C)
        K.dwconv7_idx_fwd(x.view(B, side, side, C), kept, self.s.w(p + "dw.weight"),
                          self.s.w(p + "dw.bias"), c.view(kept.Bk, side, side, C))
        n = self._e(Rk, C)
        m, r = self._e(Rk, dtype=F32), self._e(Rk, dtype=F32)
        K.mlm_ln_fwd(c, self.s.p(p + "ln.weight"), self.s.p(p + "ln.bias"), self.cfg.convnext.eps,
                     n, m, r)
        pre, act = self._e(Rk, 4 * C), self._e(Rk, 4 * C)
        self._linear(n, p + "fc1", out=pre, epi=K.EPI_BF16_GELU, out2=act)
        y = self._linear(act, p + "fc2")
        xn = self._e(R, C, dtype=F32)
        K.droppath_add_fwd(x.view(B, rps, C), self.s.p(p + "gamma"), y, kept, pj,
                           xn.view(B, rps, C))
        return xn, (x, c, m, r, n, pre, act, y, kept, pj)

    def _cn_block_drop_bwd(self, p, g, saved, B, side):
        """Backward of _cn_block_drop_fwd: only the kept planes of g change; a block that kept
        nobody (saved None) leaves g and its parameter gradients untouched."""
        if saved is None:
            return g
        x, c, m, r, n, pre, act, y, kept, pj = saved
        R, C = x.shape
        rps = side * side
        Rk = kept.Bk * rps
        self._side_fence()
        dy = self._e(Rk, C)
        K.droppath_bwd(g.view(B, rps, C), kept, self.s.p(p + "gamma"), y, pj, dy,
                       self.s.g(p + "gamma"))
        dpre = self._dx_dgelu(dy, p + "fc2", pre, bias_of=p + "fc1")
        self._dw(dy, act, p + "fc2")
        dn = self._dx(dpre, p + "fc1")
        self._dw(dpre, n, p + "fc1", bias=False)
        dc = self._e(Rk, C)
        K.ln16_bwd(c, m, r, self.s.p(p + "ln.weight"), dn, dc, dw=self.s.g(p + "ln.weight"),
                   db=self.s.g(p + "ln.bias"))
        dc4 = dc.view(kept.Bk, side, side, C)
        K.dwconv7_idx_bwd_weight(x.view(B, side, side, C), kept, dc4, self.s.g(p + "dw.weight"),
                                 self.s.g(p + "dw.bias"))
        g4 = g.view(B, side, side, C)
        K.dwconv7_idx_bwd_input(dc4, kept, self.s.w(p + "dw.weight"), g4, dx_in=g4)
        return g

    def _cn_block_fwd(self, p, x, B, side):
        """ConvNextLayer under autocast: x + gamma * f32(fc2(gelu(fc1(LN(dwconv(bf16 x))))))."""
        R, C = x.shape
        eps = self.cfg.convnext.eps
        c = self._e(R, C)
        K.dwconv7_fwd(x.view(B, side, side, C), self.s.w(p + "dw.weight"), self.s.w(p + "dw.bias"),
                      c.view(B, side, side, C))
        n = self._e(R, C)
        m, r = self._e(R, dtype=F32), self._e(R, dtype=F32)
        K.mlm_ln_fwd(c, self.s.p(p + "ln.weight"), self.s.p(p + "ln.bias"), eps, n, m, r)
        pre, act = self._e(R, 4 * C), self._e(R, 4 * C)
        self._linear(n, p + "fc1", out=pre, epi=K.EPI_BF16_GELU, out2=act)
        y = self._linear(act, p + "fc2")
        xn = self._e(R, C, dtype=F32)
        K.layerscale_add_fwd(x, self.s.p(p + "gamma"), y, xn)
        return xn, (x, c, m, r, n, pre, act, y)

    def _cn_block_bwd(self, p, g, saved, B, side):
        """g: the fp32 gradient of the block's output, overwritten by its input's."""
        x, c, m, r, n, pre, act, y = saved
        R, C = x.shape
        self._side_fence()
        dy = self._e(R, C)
        K.layerscale_bwd(g, self.s.p(p + "gamma"), y, dy, self.s.g(p + "gamma"))
        dpre = self._dx_dgelu(dy, p + "fc2", pre, bias_of=p + "fc1")
        self._dw(dy, act, p + "fc2")
        dn = self._dx(dpre, p + "fc1")
        self._dw(dpre, n, p + "fc1", bias=False)
        dc = self._e(R, C)
        K.ln16_bwd(c, m, r, self.s.p(p + "ln.weight"), dn, dc, dw=self.s.g(p + "ln.weight"),
                   db=self.s.g(p + "ln.bias"))
        dc4 = dc.view(B, side, side, C)
        K.dwconv7_bwd_weight(x.view(B, side, side, C), dc4, self.s.g(p + "dw.weight"),
                             self.s.g(p + "dw.bias"))
        g4 = g.view(B, side, side, C)
        K.dwconv7_bwd_input(dc4, self.s.w(p + "dw.weight"), g4, dx_in=g4)
        return g

    def _cn_stage_fwd(self, s, x, B, _S=None):
        """ConvNextStage s: LayerNorm + 2x2/s2 conv (s >= 1), then its blocks."""
        cn = self.cfg.convnext
        C, side = cn.hidden_sizes[s], cn.side(s)
        p = f"convnext.stages.{s}."
        ckpt = self.checkpointing and not self._recomputing
        x_in, down = x, None
        if s > 0:
            Cin, sin = cn.hidden_sizes[s - 1], cn.side(s - 1)
            yln = self._e(x.shape[0], Cin)
            m, r = self._e(x.shape[0], dtype=F32), self._e(x.shape[0], dtype=F32)
            K.layernorm_fwd(x, self.s.p(p + "down_ln.weight"), self.s.p(p + "down_ln.bias"), cn.eps,
                            yln, m, r)
            rows = self._e(B * side * side, 4 * Cin)
            K.patchify2_nhwc(yln.view(B, sin, sin, Cin), rows)
            down = (x, m, r, rows)
            x = self._cn_f32_of_bf16(rows, p + "down")
        blocks = []
        j0 = sum(cn.depths[:s])  # block numbers count over all stages (the drop-path rates)
        for j in range(cn.depths[s]):
            if self._pdp is not None and self._pdp[j0 + j] > 0:
                x, saved = self._cn_block_drop_fwd(f"{p}layers.{j}.", x, B, side, j0 + j)
            else:
                x, saved = self._cn_block_fwd(f"{p}layers.{j}.", x, B, side)
            blocks.append(saved)
        if ckpt:
            self.cache[("cn", s)] = ("ckpt", x_in)
        else:
            self.cache[("cn", s)] = (down, blocks)
        return x

    def _cn_stage_bwd(self, s, g, B):
        cn = self.cfg.convnext
        C, side = cn.hidden_sizes[s], cn.side(s)
        p = f"convnext.stages.{s}."
        self._unit_bwd(f"convnext.stages.{s}")
        self._restore(("cn", s), self._cn_stage_fwd, s, B, None)
        down, blocks = self.cache.pop(("cn", s))
        j0 = sum(cn.depths[:s])
        for j in reversed(range(cn.depths[s])):
            if self._pdp is not None and self._pdp[j0 + j] > 0:
                g = self._cn_block_drop_bwd(f"{p}layers.{j}.", g, blocks.pop(), B, side)
            else:
                g = self._cn_block_bwd(f"{p}layers.{j}.", g, blocks.pop(), B, side)
        if down is not None:
            x, m, r, rows = down
            Cin, sin = cn.hidden_sizes[s - 1], cn.side(s - 1)
            dq = self._e(g.shape[0], C)  # the stage-entry gradient, rounded to bf16 once
            K.cast_f32_bf16(g, dq)
            drows = self._dx(dq, p + "down")
            self._dw(dq, rows, p + "down")
            dyln = self._e(x.shape[0], Cin, dtype=F32)
            K.unpatchify2_nhwc(drows, dyln.view(B, sin, sin, Cin))
            g = self._e(x.shape[0], Cin, dtype=F32)
            K.layernorm_f32_bwd(x, m, r, dyln, self.s.p(p + "down_ln.weight"), g,
                                self.s.g(p + "down_ln.weight"), self.s.g(p + "down_ln.bias"))
        self._unit_done(f"convnext.stages.{s}")
        self._ready((p,))
        return g

    def _convnext_forward(self, batch: Batch, grad_scale: float, need_grad: bool) -> torch.Tensor:
        """ConvNextForImageClassification: 4x4/s4 stem + LayerNorm, the four stages, the global
        average pool, LayerNorm (head_eps), the classifier with its bias, Σ_images CE."""
        cfg, cn = self.cfg, self.cfg.convnext
        B, C0, C3 = batch.B, cn.hidden_sizes[0], cn.hidden_sizes[-1]
        self._begin(batch, need_grad)
        R0 = B * cn.side(0) ** 2
        cols = self._e(R0, cn.patch_k)
        K.im2col(batch.pixels, cn.patch, cols)
        self._unit_fwd("convnext.stem")
        po = self._cn_f32_of_bf16(cols, "convnext.stem")
        x = self._e(R0, C0, dtype=F32)
        m0, r0 = self._e(R0, dtype=F32), self._e(R0, dtype=F32)
        K.layernorm_f32_fwd(po, self.s.p("convnext.stem_ln.weight"),
                            self.s.p("convnext.stem_ln.bias"), cn.eps, x, m0, r0)
        for s in range(4):
            self._unit_fwd(f"convnext.stages.{s}")
            x = self._cn_stage_fwd(s, x, B)
        HW = cn.side(3) ** 2
        pooled = self._e(B, C3, dtype=F32)
        K.avgpool_fwd(x.view(B, HW, C3), pooled)
        y = self._e(B, C3)
        m, r = self._e(B, dtype=F32), self._e(B, dtype=F32)
        K.layernorm_fwd(pooled, self.s.p("convnext.ln_post.weight"),
                        self.s.p("convnext.ln_post.bias"), cn.head_eps, y, m, r)
        self._unit_fwd("cls_head")
        logits = self._linear(y, "cls_head")
        self.cache["head"] = (pooled, m, r, y, logits)
        self.cache["stem"] = (cols, po, m0, r0)
        return self._loss(logits, batch, cfg.num_classes, grad_scale, need_grad)

    def _convnext_backward(self, batch: Batch, scale: torch.Tensor | None) -> None:
        cn = self.cfg.convnext
        B, C0, C3 = batch.B, cn.hidden_sizes[0], cn.hidden_sizes[-1]
        pooled, m, r, y, dlogits = self._begin_backward(batch, scale)
        cols, po, m0, r0 = self.cache.pop("stem")
        self._unit_bwd("cls_head")
        dy = self._dx(dlogits, "cls_head")
        self._dw(dlogits, y, "cls_head")  # + the classifier's bias gradient
        self._unit_done("cls_head")
        del dlogits
        dp = self._e(B, C3, dtype=F32)
        K.layernorm_bwd(pooled, m, r, dy, self.s.p("convnext.ln_post.weight"), dp,
                        self.s.g("convnext.ln_post.weight"), self.s.g("convnext.ln_post.bias"))
        HW = cn.side(3) ** 2
        g = self._e(B * HW, C3, dtype=F32)
        K.avgpool_bwd(dp, g.view(B, HW, C3))
        self._ready(("cls_head.", "convnext.ln_post."))
        for s in reversed(range(4)):
            g = self._cn_stage_bwd(s, g, B)
        # the stem: its LayerNorm read the bf16 conv output, whose gradient is bf16
        self._side_fence()
        self._unit_bwd("convnext.stem")
        dpo = torch.empty_like(g)
        K.layernorm_f32_bwd(po, m0, r0, g, self.s.p("convnext.stem_ln.weight"), dpo,
                            self.s.g("convnext.stem_ln.weight"), self.s.g("convnext.stem_ln.bias"))
        dpb = self._e(g.shape[0], C0)
        K.cast_f32_bf16(dpo, dpb)
        self._dw(dpb, cols, "convnext.stem")
        self._unit_done("convnext.stem")
        self._ready(("convnext.stem.", "convnext.stem_ln."))
        self._finish()

    # -------------------------------------------------------------- RoBERTa (post-LN encoder)
    # The stream between sub-layers is fp32 AND normalised: each sub-layer ends in
    # LayerNorm(dropout(branch) + input) (include/mmpt.h K20).  A layer's input is the pair
    # (h32, h16 = bf16(h32)): h32 feeds the residual add, h16 the GEMMs.  Kept for the backward,
    # per sub-layer: the sum s the LayerNorm read (fp32), its statistics and its bf16 output; the
    # fp32 output lives only until the next add.  Attention is _attention_fwd / _bwd over the
    # planar layout; _roberta_forward / _backward are the family's body inside the step frame.
    def _roberta_layer_fwd(self, i, x, B, S):
        """RobertaLayer (tf:models/roberta/modeling_roberta.py) under autocast:
        h1 = LN1(f32(drop(dense(attn(bf16 x)))) + x);  h2 = LN2(f32(drop(fc2(gelu(fc1(bf16 h1))))) + h1)."""
        t = self.cfg.text
        x32, x16 = x
        T, h, H = x32.shape[0], t.hidden, t.heads
        p = f"text.layers.{i}."
        pt, seed = self._pt, self.dropout_seed
        ckpt = self.checkpointing and not self._recomputing
        qkv = self._linear(x16, p + "qkv")
        a = self._e(T, h)
        lse = self._e(B * H * S, dtype=F32)
        self._attention_fwd(self._attn_t, 1 + i, self._pat, qkv, B, S, a, lse, vl=self._vl)
        ao = self._linear(a, p + "dense")
        # the sum may overwrite the input stream unless that is this layer's checkpoint
        s1 = self._e(T, h, dtype=F32) if ckpt else x32
        h1, y1 = self._e(T, h, dtype=F32), self._e(T, h)
        m1, r1 = self._e(T, dtype=F32), self._e(T, dtype=F32)
        K.add_layernorm_fwd(x32, ao, self.s.p(p + "ln1.weight"), self.s.p(p + "ln1.bias"), t.eps,
                            s1, h1, y1, m1, r1, pt, seed, self._site(1 + i, 0))
        pre, act = self._e(T, t.ffn), self._e(T, t.ffn)
        self._linear(y1, p + "fc1", out=pre, epi=K.EPI_BF16_GELU, out2=act)
        mo = self._linear(act, p + "fc2")
        h2, y2 = self._e(T, h, dtype=F32), self._e(T, h)
        m2, r2 = self._e(T, dtype=F32), self._e(T, dtype=F32)
        K.add_layernorm_fwd(h1, mo, self.s.p(p + "ln2.weight"), self.s.p(p + "ln2.bias"), t.eps,
                            h1, h2, y2, m2, r2, pt, seed, self._site(1 + i, 1))  # s2 over h1
        if ckpt:
            self.cache[("t", i)] = ("ckpt", x)
        else:
            self.cache[("t", i)] = (x16, qkv, a, lse, s1, m1, r1, y1, pre, act, h1, m2, r2)
        return h2, y2

    def _roberta_layer_bwd(self, i, d32, dyb, B, S):
        """d32: the fp32 gradient of the layer's output from the residual add above (None for the
        top layer); dyb: the bf16 input gradient of the GEMM that read its bf16 copy.  Returns the
        same pair for the layer's input."""
        t = self.cfg.text
        T, h = dyb.shape[0], t.hidden
        p = f"text.layers.{i}."
        pt, seed = self._pt, self.dropout_seed
        self._side_fence()
        self._unit_bwd(f"text.layers.{i}")
        self._restore(("t", i), self._roberta_layer_fwd, i, B, S)
        x16, qkv, a, lse, s1, m1, r1, y1, pre, act, s2, m2, r2 = self.cache.pop(("t", i))
        g = self.s.g
        ds = self._e(T, h, dtype=F32) if d32 is None else d32
        dm = self._e(T, h)  # drop(bf16(ds2)): fc2's output gradient; + fc2.bias's gradient
        K.add_layernorm_bwd(s2, m2, r2, self.s.p(p + "ln2.weight"), ds, dm, dy32=d32, dyb=dyb,
                            dw=g(p + "ln2.weight"), db=g(p + "ln2.bias"), dsum=g(p + "fc2.bias"),
                            p=pt, seed=seed, site=self._site(1 + i, 1))
        dpre = self._dx_dgelu(dm, p + "fc2", pre, bias_of=p + "fc1")
        self._dw(dm, act, p + "fc2", bias=False)
        dy1 = self._dx(dpre, p + "fc1")
        self._dw(dpre, y1, p + "fc1", bias=False)
        do = self._e(T, h)  # drop(bf16(ds1)): dense's output gradient; + dense.bias's gradient
        K.add_layernorm_bwd(s1, m1, r1, self.s.p(p + "ln1.weight"), ds, do, dy32=ds, dyb=dy1,
                            dw=g(p + "ln1.weight"), db=g(p + "ln1.bias"), dsum=g(p + "dense.bias"),
                            p=pt, seed=seed, site=self._site(1 + i, 0))
        da = self._dx(do, p + "dense")
        self._dw(do, a, p + "dense", bias=False)
        dqkv = self._e(T, 3 * h)
        self._attention_bwd(self._attn_t, 1 + i, self._pat, qkv, B, S, a, da, lse, dqkv,
                            vl=self._vl)
        dx16 = self._dx(dqkv, p + "qkv")
        self._dw(dqkv, x16, p + "qkv")
        self._unit_done(f"text.layers.{i}")
        return ds, dx16

    def _roberta_forward(self, batch: Batch, grad_scale: float, need_grad: bool) -> torch.Tensor:
        """RobertaForMaskedLM: embeddings (gather + LayerNorm + dropout, one kernel), the post-LN
        layers, then the MLM head on the labelled rows only: dense + GELU, LayerNorm, the decoder
        (the tied embedding) with its bias, Σ CE over the real vocabulary."""
        t = self.cfg.text
        B, S, T, h = batch.B, batch.max_len, batch.T, t.hidden
        self._begin(batch, need_grad)
        h32, h16 = self._e(T, h, dtype=F32), self._e(T, h)
        m0, r0 = self._e(T, dtype=F32), self._e(T, dtype=F32)
        K.roberta_embed_fwd(batch.ids, batch.pos_ids, self.s.p("text.embed"),
                            self.s.p("text.pos_embed"), self.s.p("text.type_embed")[0],
                            self.s.p("text.embed_ln.weight"), self.s.p("text.embed_ln.bias"), t.eps,
                            h32, h16, m0, r0, self._pt, self.dropout_seed, self._site(0, 0),
                            noise=self._noise)
        x = (h32, h16)
        for i in range(t.layers):
            self._unit_fwd(f"text.layers.{i}")
            x = self._roberta_layer_fwd(i, x, B, S)
        self._unit_fwd("text.mlm")
        xv = self._scored_rows(x[1], batch)  # the head reads the labelled rows only
        R = xv.shape[0]
        pre, gl = self._e(R, h), self._e(R, h)
        self._linear(xv, "text.mlm.dense", out=pre, epi=K.EPI_BF16_GELU, out2=gl)
        n16 = self._e(R, h)
        mh, rh = self._e(R, dtype=F32), self._e(R, dtype=F32)
        K.mlm_ln_fwd(gl, self.s.p("text.mlm.ln.weight"), self.s.p("text.mlm.ln.bias"), t.eps, n16,
                     mh, rh)
        logits = self._e(R, t.vocab)
        K.gemm(n16, self.s.w("text.embed"), logits, bias=self.s.w("text.mlm.bias"))
        self.cache["head"] = (xv, pre, gl, mh, rh, n16, logits)
        self.cache["emb"] = (m0, r0)
        return self._loss(logits, batch, t.n_vocab, grad_scale, need_grad)

    def _roberta_backward(self, batch: Batch, scale: torch.Tensor | None) -> None:
        t = self.cfg.text
        B, S, h = batch.B, batch.max_len, t.hidden
        xv, pre, gl, mh, rh, n16, dlogits = self._begin_backward(batch, scale)
        m0, r0 = self.cache.pop("emb")
        g = self.s.g
        self._unit_bwd("text.mlm")
        dn = self._dx(dlogits, "text.embed")  # through E^T (the decoder is the tied embedding)
        self._dw(dlogits, n16, "text.embed", bias=False)
        K.colsum(dlogits, g("text.mlm.bias"), accumulate=True)
        del dlogits
        dpre = self._e(xv.shape[0], h)
        K.mlm_ln_bwd(gl, mh, rh, self.s.p("text.mlm.ln.weight"), dn, pre, dpre,
                     dw=g("text.mlm.ln.weight"), db=g("text.mlm.ln.bias"),
                     dsum=g("text.mlm.dense.bias"))
        dyb = self._dx(dpre, "text.mlm.dense")
        self._dw(dpre, xv, "text.mlm.dense", bias=False)
        self._unit_done("text.mlm")
        dyb = self._all_rows(dyb, batch)
        d32 = None
        for i in reversed(range(t.layers)):
            d32, dyb = self._roberta_layer_bwd(i, d32, dyb, B, S)
        # the embeddings: dropout and LayerNorm backward over the re-gathered sum, the type row's
        # gradient, then the two tables' deterministic scatter-adds (padding_idx rows skipped)
        K.roberta_embed_bwd(batch.ids, batch.pos_ids, self.s.p("text.embed"),
                            self.s.p("text.pos_embed"), self.s.p("text.type_embed")[0], m0, r0,
                            self.s.p("text.embed_ln.weight"), d32, d32, dhb=dyb,
                            dw=g("text.embed_ln.weight"), db=g("text.embed_ln.bias"),
                            dtype=g("text.type_embed")[0], p=self._pt, seed=self.dropout_seed,
                            site=self._site(0, 0), noise=self._noise)
        if self._side is not None:  # the tied decoder's weight gradient also lands in text.embed
            torch.cuda.current_stream(self.dev).wait_stream(self._side)
        K.embed_bwd(batch.segments, d32, g("text.embed"))
        K.embed_bwd(batch.pos_segments, d32, g("text.pos_embed"))
        self._ready(("text.",))
        self._finish()

    # -------------------------------------------------------------- mamba
    # The blocks only: around them Mamba is the causal-LM step below (_causal_forward / _backward).
    _scan_keep = True  # the forward in flight hands the scan's chunk states to a backward

    def _mamba_conv(self, ops, S, bwd=False, **kw):
        """The causal conv over `ops`, forward or backward: dense rows of S tokens, or, for packed
        rows, the varlen entry — each sequence on its own, by Batch.pos."""
        if self._vl is None:
            (K.causal_conv1d_bwd if bwd else K.causal_conv1d_fwd)(*ops, S, **kw)
        else:
            (K.causal_conv1d_varlen_bwd if bwd else K.causal_conv1d_varlen_fwd)(
                *ops, self._vl.pos, **kw)

    def _mamba_scan(self, ops, S, bwd=False, **kw):
        """The selective scan over `ops`, likewise (packed rows: by Batch.scan_tables)."""
        if self._vl is None:
            (K.selective_scan_bwd if bwd else K.selective_scan_fwd)(*ops, S, **kw)
        else:
            (K.selective_scan_varlen_bwd if bwd else K.selective_scan_varlen_fwd)(
                *ops, self._vl.scan_tables, **kw)

    def _mamba_layer_fwd(self, i, x, B, S):
        """MambaBlock (tf:models/mamba/modeling_mamba.py) with the fused arithmetic of the
        reference's fast path: x' = x + bf16(out_proj(scan(silu(conv(xs)), ...) * silu(z))) with
        xs | z = in_proj(RMS x), dt | B | C = x_proj(u), dt_raw = dt_proj.weight · dt (the bias is
        added inside the scan, in fp32)."""
        t = self.cfg.text
        T, h, I, R, N = x.shape[0], t.hidden, t.d_inner, t.rank, t.d_state
        p = f"text.layers.{i}."
        y, r = self._e(T, h), self._e(T, dtype=F32)
        K.rmsnorm_fwd(x, self.s.p(p + "norm.weight"), t.eps, y, r)
        xz = self._linear(y, p + "in_proj", bias=False)
        u = self._e(T, I)
        vl = self._vl
        self._mamba_conv((xz[:, :I], self.s.w(p + "conv.weight"), self.s.w(p + "conv.bias"), u), S)
        proj = self._linear(u, p + "x_proj", bias=False)
        dt = self._e(T, I)
        K.gemm(proj[:, :R], self.s.w(p + "dt_proj.weight"), dt)
        ckpt = self.checkpointing and not self._recomputing
        states = None
        if self._scan_keep and not ckpt:
            states = K.scan_states(B, S, I, N, self.dev) if vl is None else \
                K.scan_varlen_states(vl.scan_tables, I, N, self.dev)
        ys = self._e(T, I)
        scan = (u, dt, self.s.p(p + "dt_proj.bias"), self.s.p(p + "A_log"), proj[:, R:R + N],
                proj[:, R + N:], self.s.p(p + "D"), xz[:, I:], ys)
        self._mamba_scan(scan, S, states=states)
        xn = self._linear(ys, p + "out_proj", bias=False, epi=K.EPI_F32_RESID, out2=x)
        if ckpt:
            self.cache[("t", i)] = ("ckpt", x)
        else:
            self.cache[("t", i)] = (x, r, y, xz, u, proj, dt, ys, states)
        return xn

    def _mamba_layer_bwd(self, i, dxn, ds, B, S):
        """dxn: fp32 gradient of block i's output, ds = bf16(dxn) (out_proj's output gradient).
        Returns (dx, bf16(dx)) for block i-1."""
        t = self.cfg.text
        T, h, I, R, N = dxn.shape[0], t.hidden, t.d_inner, t.rank, t.d_state
        p = f"text.layers.{i}."
        g = self.s.g
        self._side_fence()
        self._unit_bwd(f"text.layers.{i}")
        self._restore(("t", i), self._mamba_layer_fwd, i, B, S)
        x, r, y, xz, u, proj, dt, ys, states = self.cache.pop(("t", i))
        dys = self._dx(ds, p + "out_proj")
        self._dw(ds, ys, p + "out_proj", bias=False)
        dxz, dproj = self._e(T, 2 * I), self._e(T, R + 2 * N)
        du, ddt = self._e(T, I), self._e(T, I)
        scan = (u, dt, self.s.p(p + "dt_proj.bias"), self.s.p(p + "A_log"), proj[:, R:R + N],
                proj[:, R + N:], self.s.p(p + "D"), xz[:, I:], dys, du, dxz[:, I:], ddt,
                dproj[:, R:R + N], dproj[:, R + N:], g(p + "A_log"), g(p + "D"),
                g(p + "dt_proj.bias"))
        self._mamba_scan(scan, S, bwd=True, states=states)
        K.gemm(ddt, self.s.wt(p + "dt_proj.weight"), dproj[:, :R])
        self._dw(ddt, proj[:, :R], p + "dt_proj", bias=False)
        # u feeds the scan and x_proj: the conv's backward sums the two gradients in fp32
        du2 = self._dx(dproj, p + "x_proj")
        self._dw(dproj, u, p + "x_proj", bias=False)
        conv = (xz[:, :I], self.s.w(p + "conv.weight"), self.s.w(p + "conv.bias"), du, dxz[:, :I],
                g(p + "conv.weight"), g(p + "conv.bias"))
        self._mamba_conv(conv, S, bwd=True, du2=du2)
        dy = self._dx(dxz, p + "in_proj")
        self._dw(dxz, y, p + "in_proj", bias=False)
        nxt = self._e(T, h) if i > 0 else None
        K.rmsnorm_bwd(x, r, dy, self.s.p(p + "norm.weight"), dxn, dw=self._gw(p + "norm"),
                      dresid=dxn, dx_bf16=nxt)
        self._unit_done(f"text.layers.{i}")
        return dxn, nxt

    # -------------------------------------------------------------- causal LMs
    # GPTNeoX, Llama and Mamba, text-only or (the first two) behind the ViT and the projector:
    # the embedding gather, the arch's layers (self._layer), the final LayerNorm (GPTNeoX) or
    # RMSNorm, the lm_head — tied to the embedding or not — over the scored rows, Σ CE over the
    # shifted labels.
    def _causal_forward(self, batch: Batch, grad_scale: float, need_grad: bool) -> torch.Tensor:
        cfg, t = self.cfg, self.cfg.text
        # S: the longest sequence — the padded width on the dense path, where T = B * S
        B, S, T = batch.B, batch.max_len, batch.T
        self._begin(batch, need_grad)
        img = self._vision_fwd(batch.pixels, B) if cfg.multimodal else None
        h = self._e(T, t.hidden, dtype=F32)
        self._f32_fwd("text.embed")
        # (NEFTune noise on the text rows first, then the dropout: HF's hook sits on embed_in)
        K.embed_fwd(batch.ids, self.s.p("text.embed"), h, batch.img_map, img, noise=self._noise)
        if self._pt > 0:  # GPTNeoX emb_dropout, after the image-token merge
            K.dropout_f32(h, h, self._pt, self.dropout_seed, self._site(0, 0))
        self._scan_keep = need_grad  # (Mamba: a forward without gradients keeps no scan states)
        for i in range(t.layers):
            self._unit_fwd(f"text.layers.{i}")
            h = self._layer[0](i, h, batch.n_seq, S)  # (sequences: the documents of packed rows)
        self._scan_keep = True  # a checkpoint recompute runs for a backward
        yf, mf, rf = self._e(T, t.hidden), None, self._e(T, dtype=F32)
        if t.llama or t.mamba:
            K.rmsnorm_fwd(h, self.s.p("text.final_ln.weight"), t.eps, yf, rf)
        else:
            mf = self._e(T, dtype=F32)
            K.layernorm_fwd(h, self.s.p("text.final_ln.weight"), self.s.p("text.final_ln.bias"),
                            t.eps, yf, mf, rf)
        yf = self._scored_rows(yf, batch)  # (LLaVA batches: the image slots carry no label)
        logits = self._e(yf.shape[0], t.vocab)
        if self.head == "text.lm_head":
            self._unit_fwd("text.lm_head")
        K.gemm(yf, self.s.w(self.head), logits)
        self.cache["head"] = (h, mf, rf, yf, logits)
        return self._loss(logits, batch, t.n_vocab, grad_scale, need_grad)

    def _causal_backward(self, batch: Batch, scale: torch.Tensor | None) -> None:
        cfg, t = self.cfg, self.cfg.text
        B, S, T = batch.B, batch.max_len, batch.T
        hL, mf, rf, yf, dlogits = self._begin_backward(batch, scale)
        tied = self.head == "text.embed"
        if not tied:
            self._unit_bwd("text.lm_head")
        dyf = self._dx(dlogits, self.head)
        self._dw(dlogits, yf, self.head, bias=False)
        if not tied:
            self._unit_done("text.lm_head")
        del dlogits
        dyf = self._all_rows(dyf, batch)
        dh = torch.empty_like(hL)
        if t.llama or t.mamba:
            ds = self._e(T, t.hidden)
            K.rmsnorm_bwd(hL, rf, dyf, self.s.p("text.final_ln.weight"), dh,
                          dw=self._gw("text.final_ln"), dx_bf16=ds)
        else:
            top = self._resid_grad_targets(t.layers - 1, T)
            K.layernorm_bwd(hL, mf, rf, dyf, self.s.p("text.final_ln.weight"), dh,
                            self.s.g("text.final_ln.weight"), self.s.g("text.final_ln.bias"), **top)
            ds = top["dx_bf16"]
        self._ready(("text.final_ln.",) + (() if tied else ("text.lm_head",)))
        for i in reversed(range(t.layers)):
            dh, ds = self._layer[1](i, dh, ds, batch.n_seq, S)
            self._ready((f"text.layers.{i}.",))
        dimg = self._e(B * cfg.vision.num_patches, t.hidden) if cfg.multimodal else None
        if self._pt > 0:
            K.dropout_f32(dh, dh, self._pt, self.dropout_seed, self._site(0, 0))
        # the tied decoder's weight gradient also lands in text.embed: Mamba waits for it here
        # (GPTNeoX and Llama leave that order to the layers' _side_fence, as they always have)
        if t.mamba and self._side is not None:
            torch.cuda.current_stream(self.dev).wait_stream(self._side)
        self._f32_bwd("text.embed")
        K.embed_bwd(batch.segments, dh, None if self.frozen else self.s.g("text.embed"),
                    batch.img_map, dimg)
        self._f32_done("text.embed")
        self._ready(("text.embed",))
        if cfg.multimodal:
            self._vision_bwd(dimg, B)
            self._ready(("vision.", "proj."))
        self._finish()

    # -------------------------------------------------------------- whole model
    def forward(self, batch: Batch, grad_scale: float, need_grad: bool = True) -> torch.Tensor:
        """Returns Σ_tokens CE (device fp32 [1]); when need_grad, dlogits are written
        (scaled by grad_scale = 1/num_items of the global batch) and the caches kept."""
        return self._family[0](batch, grad_scale, need_grad)

    def backward(self, batch: Batch, scale: torch.Tensor | None = None) -> None:
        """Accumulates every parameter gradient into the flat grad buffer.  `scale`
        (device scalar, e.g. autograd's grad_output) multiplies the loss gradient."""
        self._family[1](batch, scale)

