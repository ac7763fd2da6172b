"""Model configurations of the hot path (product-owned; no HF import).

Hyper-parameters restate the public HF configs the reference loads by name
(GPTNeoXConfig.from_pretrained("EleutherAI/pythia-*"), src/models/pythia.py:18-21;
ViTConfig, src/models/vit.py:11-16) — they cannot be fetched offline, so they
are written out here (SURVEY.md §8c "Unavailable offline").
"""

from __future__ import annotations

from dataclasses import dataclass, replace


def _check_dropout(p: float, where: str, field: str = "hidden_dropout") -> None:
    if not 0.0 <= p < 1.0:
        raise ValueError(f"{where}.{field} must lie in [0, 1), got {p!r}")


@dataclass(frozen=True)
class VisionConfig:
    """ViT encoder (tf:models/vit): pre-LN, qkv bias, erf-GELU, LN eps 1e-12."""

    hidden: int = 768
    layers: int = 12
    heads: int = 12
    ffn: int = 3072
    image: int = 224
    patch: int = 16
    channels: int = 3
    eps: float = 1e-12
    feature_layer: int = -2  # LlavaConfig.vision_feature_layer default
    # CLIP vision tower (tf:models/clip/modeling_clip.py; the reference's llava-pretrain
    # tower openai/clip-vit-large-patch14-336, src/models/llava.py:24-45): quick-GELU MLP,
    # pre_layrnorm on the embeddings, bias-free patch conv, LN eps 1e-5
    act: str = "gelu"  # "gelu" (erf) | "quick_gelu"
    pre_ln: bool = False
    patch_bias: bool = True
    # ViTConfig.hidden_dropout_prob: ViTEmbeddings.dropout, ViTSelfOutput.dropout and
    # ViTOutput.dropout in training mode.  The ViT tower only: CLIP has no hidden dropout
    hidden_dropout: float = 0.0
    # ViTConfig.attention_probs_dropout_prob / CLIPVisionConfig.attention_dropout: dropout on the
    # softmax output in training mode, inside the flash-attention kernels (include/mmpt.h K19;
    # the probability is quantised to floor(p * 256) / 256)
    attention_dropout: float = 0.0

    def __post_init__(self):
        _check_dropout(self.hidden_dropout, "VisionConfig")
        _check_dropout(self.attention_dropout, "VisionConfig", "attention_dropout")
        if self.hidden_dropout > 0 and self.pre_ln:
            raise ValueError("hidden_dropout > 0 on a CLIP tower (pre_ln): CLIPVisionConfig has "
                             "no hidden dropout")

    @property
    def patch_k(self) -> int:
        """im2col width C·p·p padded to a multiple of 8 (16-B GEMM rows; zero columns)."""
        return (self.channels * self.patch * self.patch + 7) // 8 * 8

    @property
    def num_patches(self) -> int:
        return (self.image // self.patch) ** 2

    @property
    def head_dim(self) -> int:
        return self.hidden // self.heads

    @property
    def used_layers(self) -> int:
        """hidden_states[feature_layer] needs only the first L+1+feature_layer layers (P12)."""
        return self.layers + 1 + self.feature_layer


@dataclass(frozen=True)
class TextConfig:
    """arch "gptneox": GPTNeoX / Pythia (tf:models/gpt_neox) — parallel residual, LayerNorm,
    partial RoPE, fused per-head q|k|v with biases, erf-GELU MLP, untied lm_head.
    arch "llama": Llama-3 (tf:models/llama, the LLM of the reference's llava-pretrain,
    src/models/llava.py:25) — sequential residual, RMSNorm, GQA (kv_heads), full RoPE with
    the llama3 frequency scaling, SwiGLU MLP, no biases, lm_head tied to the embedding.
    arch "roberta": RoBERTa masked LM (tf:models/roberta, the reference's src/models/roberta.py) —
    post-LN encoder (LayerNorm after each residual add), learned positions counted from
    pad_id + 1 over the non-pad ids, a LayerNorm over the summed word / position / type
    embeddings, non-causal attention, erf-GELU MLP, the MLM head (dense, GELU, LayerNorm, the
    decoder tied to the embedding plus a bias of its own), no label shift.
    arch "mamba": Mamba (tf:models/mamba, the reference's src/models/mamba.py) — a stack of
    MambaBlocks: RMSNorm of the fp32 residual, then the mixer (in_proj to x | z, a causal
    depthwise conv of d_conv taps + SiLU over x, x_proj to dt | B | C, dt_proj, the selective scan
    over d_state states per channel gated by silu(z), out_proj) added back to the residual; a final
    RMSNorm and a decoder tied to the embedding.  No attention: `heads`, `ffn` and the rotary
    fields are unused.  No dropout of either kind (MambaConfig has none)."""

    hidden: int = 2048
    layers: int = 16
    heads: int = 8
    ffn: int = 8192
    vocab: int = 50304
    rotary_pct: float = 0.25
    rope_theta: float = 10000.0
    eps: float = 1e-5
    arch: str = "gptneox"
    kv_heads: int = 0  # 0 = heads (no GQA)
    # llama3 rope scaling: (factor, low_freq_factor, high_freq_factor, original_max_position)
    rope_scaling: tuple | None = None
    tie_embeddings: bool = False
    vocab_valid: int = 0  # real vocabulary when `vocab` is padded to a multiple of 8 (0 = vocab)
    # GPTNeoXConfig.hidden_dropout: emb_dropout, post_attention_dropout and post_mlp_dropout in
    # training mode.  GPTNeoX only: LlamaConfig has no hidden dropout
    hidden_dropout: float = 0.0
    # GPTNeoXConfig.attention_dropout / LlamaConfig.attention_dropout: dropout on the softmax
    # output in training mode, inside the flash-attention kernels (include/mmpt.h K19; the
    # probability is quantised to floor(p * 256) / 256).  Named attn_dropout here, not
    # attention_dropout as on VisionConfig: tests/test_dropout_cpu.py pins that a TextConfig has
    # no attribute of that name
    attn_dropout: float = 0.0
    # arch "roberta": RobertaConfig.max_position_embeddings / pad_token_id (the padding_idx of the
    # word and position tables) / type_vocab_size
    max_positions: int = 0
    pad_id: int = 1
    type_vocab: int = 1
    # arch "mamba": MambaConfig.state_size / conv_kernel / expand / time_step_rank (0 = "auto",
    # ceil(hidden / 16)); the conv has a bias, the linears have none
    d_state: int = 16
    d_conv: int = 4
    expand: int = 2
    dt_rank: int = 0

    def __post_init__(self):
        _check_dropout(self.hidden_dropout, "TextConfig")
        _check_dropout(self.attn_dropout, "TextConfig", "attn_dropout (attention_dropout)")
        if self.arch == "mamba":
            if self.hidden_dropout or self.attn_dropout:
                raise ValueError("arch 'mamba': MambaConfig has no hidden or attention dropout")
            if self.rotary_pct != 0 or not self.tie_embeddings or self.kv_heads or \
                    self.rope_scaling is not None:
                raise ValueError("arch 'mamba': rotary_pct 0, tied embeddings, no GQA, no rope scaling")
            if self.d_conv != 4 or self.d_state not in (8, 16):
                raise ValueError("arch 'mamba': d_conv 4 and d_state 8 or 16 (the scan kernels' sizes)")
            if self.expand < 1 or self.dt_rank < 0 or self.d_inner % 8 or self.rank % 8:
                raise ValueError("arch 'mamba': d_inner = expand * hidden and the dt rank must be "
                                 f"multiples of 8 (16-B GEMM rows), got {self.d_inner} and {self.rank}")
        if self.hidden_dropout > 0 and self.arch == "llama":
            raise ValueError("hidden_dropout > 0 on a Llama text model: LlamaConfig has no "
                             "hidden dropout")
        if self.arch == "roberta":
            if self.rotary_pct != 0 or not self.tie_embeddings or self.kv_heads:
                raise ValueError("arch 'roberta': rotary_pct 0, tied embeddings, no GQA")
            if self.type_vocab != 1:
                raise ValueError("arch 'roberta': type_vocab_size 1 only (token_type_ids are zero)")
            if not 0 <= self.pad_id < self.n_vocab or self.max_positions < self.pad_id + 3:
                raise ValueError("arch 'roberta': pad_id must be a vocabulary id and max_positions "
                                 "at least pad_id + 3")

    @property
    def head_dim(self) -> int:
        return self.hidden // self.heads

    @property
    def rot_dims(self) -> int:
        return int(self.head_dim * self.rotary_pct)

    @property
    def llama(self) -> bool:
        return self.arch == "llama"

    @property
    def roberta(self) -> bool:
        return self.arch == "roberta"

    @property
    def mamba(self) -> bool:
        return self.arch == "mamba"

    @property
    def d_inner(self) -> int:
        return self.expand * self.hidden

    @property
    def rank(self) -> int:
        """dt_rank, "auto" (0) resolved as MambaConfig does: ceil(hidden / 16)"""
        return self.dt_rank or -(-self.hidden // 16)

    @property
    def xproj_dim(self) -> int:
        """x_proj's rows: the low-rank dt input, then B and C"""
        return self.rank + 2 * self.d_state

    def check_seq(self, seq: int) -> None:
        """RoBERTa's position ids reach seq + pad_id: a longer sequence has no table row."""
        if self.roberta and seq + self.pad_id + 1 > self.max_positions:
            raise ValueError(f"sequence length {seq} needs {seq + self.pad_id + 1} position rows; "
                             f"max_positions is {self.max_positions}")

    @property
    def n_kv(self) -> int:
        return self.kv_heads or self.heads

    @property
    def qkv_dim(self) -> int:
        return (self.heads + 2 * self.n_kv) * self.head_dim

    @property
    def n_vocab(self) -> int:
        return self.vocab_valid or self.vocab


@dataclass(frozen=True)
class ConvNextConfig:
    """ConvNeXt (tf:models/convnext): a 4x4/s4 patch stem + LayerNorm, four stages of
    ConvNextLayer blocks (7x7 depthwise conv, LayerNorm, 4x pointwise MLP with erf-GELU, layer
    scale gamma, residual) with a LayerNorm + 2x2/s2 conv downsample in front of stages 1-3,
    then the global average pool, a LayerNorm (head_eps = ConvNextConfig.layer_norm_eps) and the
    classifier.  drop_path_rate (ConvNextConfig.drop_path_rate: stochastic depth, per-block rates
    rising linearly from 0) is 0 in every configuration the reference builds."""

    hidden_sizes: tuple = (96, 192, 384, 768)
    depths: tuple = (3, 3, 9, 3)
    image: int = 224
    patch: int = 4
    channels: int = 3
    eps: float = 1e-6
    head_eps: float = 1e-12
    layer_scale_init: float = 1e-6
    drop_path_rate: float = 0.0

    def __post_init__(self):
        _check_dropout(self.drop_path_rate, "ConvNextConfig", "drop_path_rate")
        if len(self.hidden_sizes) != 4 or len(self.depths) != 4:
            raise ValueError("ConvNextConfig: four stages (hidden_sizes and depths of length 4)")
        if any(c <= 0 or c % 8 for c in self.hidden_sizes) or any(d <= 0 for d in self.depths):
            raise ValueError("ConvNextConfig: hidden_sizes positive multiples of 8, depths >= 1")
        if self.image % (self.patch * 8):
            raise ValueError("ConvNextConfig: image must be a multiple of 8 * patch (three 2x2 "
                             "downsamples after the stem)")

    @property
    def patch_k(self) -> int:
        """im2col width C·p·p padded to a multiple of 8 (16-B GEMM rows; zero columns)."""
        return (self.channels * self.patch * self.patch + 7) // 8 * 8

    def side(self, stage: int) -> int:
        """H = W of a stage's plane."""
        return self.image // self.patch >> stage

    def drop_path_rates(self) -> tuple:
        """Drop probability of block j, counted over all stages, as HF's ConvNextEncoder has it:
        torch.linspace(0, drop_path_rate, sum(depths)).tolist() — fp32 values held as Python
        floats; block 0 is never dropped."""
        import torch
        return tuple(torch.linspace(0, self.drop_path_rate, sum(self.depths)).tolist())


@dataclass(frozen=True)
class ModelConfig:
    """text + optional vision tower: a language model or a LLaVA composition.  text = None
    with num_classes > 0: a vision-only classifier — ViTForImageClassification
    (tf:models/vit/modeling_vit.py: the encoder, vit.layernorm, the CLS row, a Linear head) over
    `vision`, or ConvNextForImageClassification over `convnext`."""

    text: TextConfig | None = None
    vision: VisionConfig | None = None
    image_token_id: int = 50303  # last id of the 50304 Pythia vocab
    # LLaVA-pretrain freeze (src/models/llava.py:49-52, under the pinned transformers 4.47.1
    # names): the vision tower and the whole language model (embeddings, layers, final norm,
    # lm_head) are frozen — only the projector is trained.
    freeze_tower_and_llm: bool = False
    num_classes: int = 0  # > 0 (with text = None): the classification head's labels
    convnext: ConvNextConfig | None = None

    def __post_init__(self):
        if self.convnext is not None:
            if self.text is not None or self.vision is not None or self.num_classes <= 0:
                raise ValueError("a ConvNeXt model is a vision-only classifier: no text model, no "
                                 "ViT tower, num_classes > 0")
            if self.freeze_tower_and_llm:
                raise ValueError("the ConvNeXt classifier has nothing frozen")
        elif self.text is None:
            if self.vision is None or self.num_classes <= 0:
                raise ValueError("a model without a text model is a vision-only classifier: it "
                                 "needs a vision tower and num_classes > 0")
            if self.vision.pre_ln or self.freeze_tower_and_llm:
                raise ValueError("the classifier is ViTForImageClassification: a ViT tower "
                                 "(no pre_ln), nothing frozen")
        elif self.num_classes:
            raise ValueError("num_classes > 0 needs text = None (a vision-only classifier)")

    @property
    def multimodal(self) -> bool:
        return self.vision is not None

    @property
    def classifier(self) -> bool:
        return self.text is None

    @property
    def classes_padded(self) -> int:
        """num_classes rounded up to a multiple of 8 (16-B GEMM rows): the pad rows of the head
        are zero, take no part in the softmax (vocab_valid) and keep a zero gradient."""
        return (self.num_classes + 7) // 8 * 8

    def trainable(self, name: str) -> bool:
        return not self.freeze_tower_and_llm or name.startswith("proj.")


def _pythia(h, L, H, F):
    return TextConfig(hidden=h, layers=L, heads=H, ffn=F)


PYTHIA = {
    "pythia-14m": _pythia(128, 6, 4, 512),
    "pythia-31m": _pythia(256, 6, 8, 1024),
    "pythia-70m": _pythia(512, 6, 8, 2048),
    "pythia-160m": _pythia(768, 12, 12, 3072),
    "pythia-410m": _pythia(1024, 24, 16, 4096),
    "pythia-1b": _pythia(2048, 16, 8, 8192),
    "pythia-1.4b": _pythia(2048, 24, 16, 8192),
    "pythia-2.8b": _pythia(2560, 32, 32, 10240),
    "pythia-6.9b": _pythia(4096, 32, 32, 16384),
    "pythia-12b": _pythia(5120, 36, 40, 20480),
}

def _llama(h, L, H, kv, F, V, V_valid, theta=500000.0, scaling=(32.0, 1.0, 4.0, 8192),
           tie=True, eps=1e-5):
    return TextConfig(hidden=h, layers=L, heads=H, kv_heads=kv, ffn=F, vocab=V, vocab_valid=V_valid,
                      rotary_pct=1.0, rope_theta=theta, eps=eps, arch="llama", rope_scaling=scaling,
                      tie_embeddings=tie)


# meta-llama/Llama-3.2-1B(-Instruct) public config (hidden 2048, 16 layers, 32 q / 8 kv heads
# of 64, SwiGLU 8192, rope_theta 5e5 with llama3 scaling factor 32 / 1 / 4 / 8192, tied
# embeddings), with the reference's added "<image>" token (src/models/llava.py:40-45:
# 128256 + 1 = 128257 ids, image token 128256) padded to 128264 rows (16-B rows; the
# padding takes no part in the softmax)
LLAMA32_1B = _llama(2048, 16, 32, 8, 8192, 128264, 128257)

VIT_B16 = VisionConfig()
CLIP_L14_336 = VisionConfig(hidden=1024, layers=24, heads=16, ffn=4096, image=336, patch=14,
                            eps=1e-5, act="quick_gelu", pre_ln=True, patch_bias=False)

PRESETS: dict[str, ModelConfig] = {name: ModelConfig(text=t) for name, t in PYTHIA.items()}
PRESETS["vit-b16-pythia-1b"] = ModelConfig(text=PYTHIA["pythia-1b"], vision=VIT_B16)
# BASELINE C5: CLIP-ViT-L/14-336 + Pythia-2.8B (576 image tokens + text)
PRESETS["clip-l14-336-pythia-2.8b"] = ModelConfig(text=PYTHIA["pythia-2.8b"], vision=CLIP_L14_336)
# the reference's own image-text model: llava-pretrain = CLIP-ViT-L/14-336 + Llama-3.2-1B
# (src/models/llava.py:22-58), freeze semantics of the pinned transformers 4.47.1
PRESETS["llava-pretrain"] = ModelConfig(text=LLAMA32_1B, vision=CLIP_L14_336, image_token_id=128256,
                                        freeze_tower_and_llm=True)
# the same composition with every parameter trained (transformers 5.x, where the freeze's
# name prefixes no longer match: SURVEY P12)
PRESETS["llava-pretrain-unfrozen"] = ModelConfig(text=LLAMA32_1B, vision=CLIP_L14_336,
                                                 image_token_id=128256)
PRESETS["llama-3.2-1b"] = ModelConfig(text=LLAMA32_1B)
# kernel-compatible tiny configs for parity tests (head_dim 64, 80-128 step 16, 256;
# dims % 8 == 0)
PRESETS["tiny-mm"] = ModelConfig(
    text=TextConfig(hidden=512, layers=2, heads=2, ffn=1024, vocab=1024),
    vision=VisionConfig(hidden=128, layers=3, heads=2, ffn=256, image=64, patch=16),
    image_token_id=1023)
# tiny-mm with hidden dropout 0.1 on both sides (with_dropout below restates it)
PRESETS["tiny-mm-drop"] = ModelConfig(
    text=replace(PRESETS["tiny-mm"].text, hidden_dropout=0.1),
    vision=replace(PRESETS["tiny-mm"].vision, hidden_dropout=0.1), image_token_id=1023)
# vision-only classifiers: the reference's `vit` (src/models/vit.py: ViT-L/16-224 in21k config,
# 21,841 labels, hidden_dropout_prob 0.1) and tiny forms for the parity tests (17 tokens per
# image, 1001 classes padded to 1008)
VIT_L16_CLS = VisionConfig(hidden=1024, layers=24, heads=16, ffn=4096, image=224, patch=16,
                           eps=1e-12, hidden_dropout=0.1, feature_layer=-1)
PRESETS["vit-l16-cls"] = ModelConfig(vision=VIT_L16_CLS, num_classes=21841)
PRESETS["tiny-vit-cls"] = ModelConfig(
    vision=VisionConfig(hidden=128, layers=3, heads=2, ffn=256, image=64, patch=16,
                        feature_layer=-1), num_classes=1001)
PRESETS["tiny-vit-cls-drop"] = ModelConfig(
    vision=replace(PRESETS["tiny-vit-cls"].vision, hidden_dropout=0.1), num_classes=1001)
# the reference's convnext-* (src/models/convnext.py: ConvNeXt-L / -XL at 224 px, ImageNet-1k or
# -22k labels) and a tiny form for the parity tests: planes 16, 8, 4, 2 (two smaller than the 7x7
# filter), channel counts that are no powers of two, a stage of three blocks
CONVNEXT_L = ConvNextConfig(hidden_sizes=(192, 384, 768, 1536), depths=(3, 3, 27, 3))
CONVNEXT_XL = ConvNextConfig(hidden_sizes=(256, 512, 1024, 2048), depths=(3, 3, 27, 3))
PRESETS["convnext-large-1k"] = ModelConfig(convnext=CONVNEXT_L, num_classes=1000)
PRESETS["convnext-large-22k"] = ModelConfig(convnext=CONVNEXT_L, num_classes=21841)
PRESETS["convnext-xlarge-22k"] = ModelConfig(convnext=CONVNEXT_XL, num_classes=21841)
PRESETS["tiny-convnext"] = ModelConfig(
    convnext=ConvNextConfig(hidden_sizes=(24, 48, 96, 192), depths=(1, 1, 3, 1), image=64),
    num_classes=1001)
PRESETS["tiny-lm"] = ModelConfig(text=TextConfig(hidden=256, layers=2, heads=2, ffn=512, vocab=512))
# Pythia-2.8B's head shape (head_dim 80 -> padded D = 128 attention, 20 rotary dims)
PRESETS["tiny-lm-d80"] = ModelConfig(text=TextConfig(hidden=320, layers=2, heads=4, ffn=640,
                                                     vocab=512))
# C5's shapes scaled down: CLIP tower (quick-GELU, pre-LN, 14-px patches) + head_dim 80
PRESETS["tiny-clip-d80"] = ModelConfig(
    text=TextConfig(hidden=320, layers=2, heads=4, ffn=640, vocab=1024),
    vision=VisionConfig(hidden=128, layers=3, heads=2, ffn=256, image=56, patch=14, eps=1e-5,
                        act="quick_gelu", pre_ln=True, patch_bias=False),
    image_token_id=1023)


# Llama-shaped tiny configs (GQA at head_dim 64, SwiGLU F % 128 == 0, padded vocab)
PRESETS["tiny-llama"] = ModelConfig(text=_llama(256, 2, 4, 1, 256, 520, 515,
                                                scaling=(32.0, 1.0, 4.0, 64)))
PRESETS["tiny-llava"] = ModelConfig(
    text=_llama(256, 2, 4, 2, 256, 1032, 1025, scaling=(32.0, 1.0, 4.0, 64)),
    vision=VisionConfig(hidden=128, layers=3, heads=2, ffn=256, image=56, patch=14, eps=1e-5,
                        act="quick_gelu", pre_ln=True, patch_bias=False),
    image_token_id=1024)
PRESETS["tiny-llava-frozen"] = ModelConfig(text=PRESETS["tiny-llava"].text,
                                           vision=PRESETS["tiny-llava"].vision,
                                           image_token_id=1024, freeze_tower_and_llm=True)


def _roberta(h, L, H, F, V, V_valid, max_pos, drop=0.0):
    return TextConfig(hidden=h, layers=L, heads=H, ffn=F, vocab=V, vocab_valid=V_valid,
                      rotary_pct=0.0, eps=1e-5, arch="roberta", tie_embeddings=True,
                      hidden_dropout=drop, attn_dropout=drop, max_positions=max_pos)


# the reference's `roberta` (src/models/roberta.py: RobertaConfig.from_pretrained("roberta-large")):
# 24 layers, hidden 1024, 16 heads of 64, FFN 4096, 514 positions, vocabulary 50265 padded to
# 50272 rows (16-B GEMM rows; the padding takes no part in the softmax), both dropouts 0.1
PRESETS["roberta-large"] = ModelConfig(text=_roberta(1024, 24, 16, 4096, 50272, 50265, 514, 0.1))
PRESETS["tiny-roberta"] = ModelConfig(text=_roberta(128, 2, 2, 256, 520, 515, 66))
PRESETS["tiny-roberta-drop"] = ModelConfig(text=_roberta(128, 2, 2, 256, 520, 515, 66, 0.1))


def _mamba(h, L, V, V_valid=0, rank=0, state=16):
    return TextConfig(hidden=h, layers=L, heads=1, ffn=0, vocab=V, vocab_valid=V_valid,
                      rotary_pct=0.0, eps=1e-5, arch="mamba", tie_embeddings=True, d_state=state,
                      d_conv=4, expand=2, dt_rank=rank)


# the reference's `mamba` (src/models/mamba.py: MambaConfig.from_pretrained(
# "state-spaces/mamba-2.8b-hf")), its published values written out: hidden 2560, 64 layers,
# d_inner 5120, 16 states, 4 taps, dt rank 160, vocabulary 50280; everything else is MambaConfig's
# default (RMSNorm eps 1e-5, conv bias, no linear biases, fp32 residual)
PRESETS["mamba-2.8b"] = ModelConfig(text=_mamba(2560, 64, 50280, rank=160))
PRESETS["tiny-mamba"] = ModelConfig(text=_mamba(128, 2, 520, 515, rank=8))


def with_dropout(cfg: ModelConfig, text: float = 0.0, vision: float = 0.0, *,
                 text_attention: float = 0.0, vision_attention: float = 0.0) -> ModelConfig:
    """`cfg` with the dropout probabilities set.  Hidden dropout: `text` on a GPTNeoX language
    model, `vision` on a ViT tower; a value > 0 where HF has no hidden dropout (Llama, a CLIP
    tower) raises ValueError.  Attention-probability dropout: `text_attention` on the language
    model (GPTNeoX or Llama; TextConfig.attn_dropout), `vision_attention` on the tower (ViT or
    CLIP; VisionConfig.attention_dropout).  Any value > 0 on a
    side the model does not have raises ValueError."""
    if cfg.vision is None:
        if vision > 0:
            raise ValueError("vision hidden_dropout > 0 on a model without a vision tower")
        if vision_attention > 0:
            raise ValueError("vision attention_dropout > 0 on a model without a vision tower")
        return replace(cfg, text=replace(cfg.text, hidden_dropout=text,
                                         attn_dropout=text_attention))
    if cfg.text is None:
        if text > 0:
            raise ValueError("text hidden_dropout > 0 on a model without a text model")
        if text_attention > 0:
            raise ValueError("text attention_dropout > 0 on a model without a text model")
        return replace(cfg, vision=replace(cfg.vision, hidden_dropout=vision,
                                           attention_dropout=vision_attention))
    return replace(cfg, text=replace(cfg.text, hidden_dropout=text, attn_dropout=text_attention),
                   vision=replace(cfg.vision, hidden_dropout=vision,
                                  attention_dropout=vision_attention))


def with_drop_path(cfg: ModelConfig, rate: float) -> ModelConfig:
    """`cfg` with ConvNextConfig.drop_path_rate set.  Only ConvNeXt has stochastic depth among the
    families here (HF's ViT, CLIP, GPTNeoX, Llama, RoBERTa and Mamba have no drop path): any
    other model raises ValueError."""
    if cfg.convnext is None:
        raise ValueError("drop_path_rate on a model without a ConvNeXt backbone: HF has no drop "
                         "path for this family")
    return replace(cfg, convnext=replace(cfg.convnext, drop_path_rate=rate))


# stochastic depth on the tiny ConvNeXt: block rates 0 .. 0.5, and 0 .. 0.8 (whole blocks with no
# sample kept at B = 2)
PRESETS["tiny-convnext-dp"] = with_drop_path(PRESETS["tiny-convnext"], 0.5)
PRESETS["tiny-convnext-dp8"] = with_drop_path(PRESETS["tiny-convnext"], 0.8)
# attention-probability dropout 0.1 (tiny-mm-adrop: hidden and attention dropout on both sides)
PRESETS["tiny-lm-adrop"] = with_dropout(PRESETS["tiny-lm"], text_attention=0.1)
PRESETS["tiny-mm-adrop"] = with_dropout(PRESETS["tiny-mm"], 0.1, 0.1, text_attention=0.1,
                                        vision_attention=0.1)
PRESETS["tiny-llama-adrop"] = with_dropout(PRESETS["tiny-llama"], text_attention=0.1)
PRESETS["tiny-vit-cls-adrop"] = with_dropout(PRESETS["tiny-vit-cls"], vision_attention=0.1)


def get_config(name: str) -> ModelConfig:
    try:
        return PRESETS[name]
    except KeyError as e:
        raise ValueError(f"unknown model {name!r}; known: {sorted(PRESETS)}") from e


def preset_name(cfg: ModelConfig) -> str | None:
    """The PRESETS key of a configuration (None: not a preset) — for messages."""
    return next((n for n, c in PRESETS.items() if c == cfg), None)


def param_shapes(cfg: ModelConfig) -> dict[str, tuple[int, ...]]:
    """The build's flat state-dict layout (HF mapping: oracle/hf_mapping.py)."""
    s: dict[str, tuple[int, ...]] = {}
    t = cfg.text
    if cfg.convnext is not None:
        cn = cfg.convnext
        s["convnext.stem.weight"] = (cn.hidden_sizes[0], cn.patch_k)
        s["convnext.stem.bias"] = (cn.hidden_sizes[0],)
        s["convnext.stem_ln.weight"] = (cn.hidden_sizes[0],)
        s["convnext.stem_ln.bias"] = (cn.hidden_sizes[0],)
        for si, (C, depth) in enumerate(zip(cn.hidden_sizes, cn.depths)):
            p = f"convnext.stages.{si}."
            if si > 0:
                Cin = cn.hidden_sizes[si - 1]
                s[p + "down_ln.weight"] = (Cin,)
                s[p + "down_ln.bias"] = (Cin,)
                s[p + "down.weight"] = (C, 4 * Cin)  # columns (ky, kx, c)
                s[p + "down.bias"] = (C,)
            for j in range(depth):
                q = f"{p}layers.{j}."
                s[q + "dw.weight"] = (49, C)             # tap-major (HF: [C, 1, 7, 7])
                s[q + "dw.bias"] = (C,)
                s[q + "ln.weight"] = (C,)
                s[q + "ln.bias"] = (C,)
                s[q + "fc1.weight"] = (4 * C, C)         # pwconv1
                s[q + "fc1.bias"] = (4 * C,)
                s[q + "fc2.weight"] = (C, 4 * C)         # pwconv2
                s[q + "fc2.bias"] = (C,)
                s[q + "gamma"] = (C,)                    # layer_scale_parameter
        s["convnext.ln_post.weight"] = (cn.hidden_sizes[-1],)
        s["convnext.ln_post.bias"] = (cn.hidden_sizes[-1],)
        s["cls_head.weight"] = (cfg.classes_padded, cn.hidden_sizes[-1])
        s["cls_head.bias"] = (cfg.classes_padded,)
        return s
    if cfg.vision is not None:
        v = cfg.vision
        s["vision.patch.weight"] = (v.hidden, v.patch_k)
        if v.patch_bias:
            s["vision.patch.bias"] = (v.hidden,)
        s["vision.cls"] = (v.hidden,)
        s["vision.pos"] = (v.num_patches + 1, v.hidden)
        if v.pre_ln:
            s["vision.ln_pre.weight"] = (v.hidden,)
            s["vision.ln_pre.bias"] = (v.hidden,)
        for i in range(v.used_layers):
            p = f"vision.layers.{i}."
            s[p + "ln1.weight"] = (v.hidden,)
            s[p + "ln1.bias"] = (v.hidden,)
            s[p + "qkv.weight"] = (3 * v.hidden, v.hidden)
            s[p + "qkv.bias"] = (3 * v.hidden,)
            s[p + "o.weight"] = (v.hidden, v.hidden)
            s[p + "o.bias"] = (v.hidden,)
            s[p + "ln2.weight"] = (v.hidden,)
            s[p + "ln2.bias"] = (v.hidden,)
            s[p + "fc1.weight"] = (v.ffn, v.hidden)
            s[p + "fc1.bias"] = (v.ffn,)
            s[p + "fc2.weight"] = (v.hidden, v.ffn)
            s[p + "fc2.bias"] = (v.hidden,)
        if cfg.classifier:  # vit.layernorm + classifier (pad rows: classes_padded)
            s["vision.ln_post.weight"] = (v.hidden,)
            s["vision.ln_post.bias"] = (v.hidden,)
            s["cls_head.weight"] = (cfg.classes_padded, v.hidden)
            s["cls_head.bias"] = (cfg.classes_padded,)
            return s
        s["proj.fc1.weight"] = (t.hidden, v.hidden)
        s["proj.fc1.bias"] = (t.hidden,)
        s["proj.fc2.weight"] = (t.hidden, t.hidden)
        s["proj.fc2.bias"] = (t.hidden,)
    s["text.embed"] = (t.vocab, t.hidden)
    if t.mamba:
        I, R, N = t.d_inner, t.rank, t.d_state
        for i in range(t.layers):
            p = f"text.layers.{i}."
            s[p + "norm.weight"] = (t.hidden,)            # MambaBlock.norm (RMS)
            s[p + "in_proj.weight"] = (2 * I, t.hidden)   # x | z
            s[p + "conv.weight"] = (t.d_conv, I)          # tap-major (HF: [I, 1, d_conv])
            s[p + "conv.bias"] = (I,)
            s[p + "x_proj.weight"] = (R + 2 * N, I)       # dt | B | C
            s[p + "dt_proj.weight"] = (I, R)
            s[p + "dt_proj.bias"] = (I,)
            s[p + "A_log"] = (I, N)
            s[p + "D"] = (I,)
            s[p + "out_proj.weight"] = (t.hidden, I)
        s["text.final_ln.weight"] = (t.hidden,)           # norm_f; the decoder is text.embed
        return s
    if t.llama:
        for i in range(t.layers):
            p = f"text.layers.{i}."
            s[p + "ln1.weight"] = (t.hidden,)             # input_layernorm (RMS)
            s[p + "qkv.weight"] = (t.qkv_dim, t.hidden)   # q_proj | k_proj | v_proj
            s[p + "dense.weight"] = (t.hidden, t.hidden)  # o_proj
            s[p + "ln2.weight"] = (t.hidden,)             # post_attention_layernorm (RMS)
            s[p + "gate_up.weight"] = (2 * t.ffn, t.hidden)  # gate|up, 128-row blocks
            s[p + "down.weight"] = (t.hidden, t.ffn)
        s["text.final_ln.weight"] = (t.hidden,)
        if not t.tie_embeddings:
            s["text.lm_head"] = (t.vocab, t.hidden)
        return s
    if t.roberta:
        s["text.pos_embed"] = (t.max_positions, t.hidden)
        s["text.type_embed"] = (t.type_vocab, t.hidden)
        s["text.embed_ln.weight"] = (t.hidden,)
        s["text.embed_ln.bias"] = (t.hidden,)
        for i in range(t.layers):
            p = f"text.layers.{i}."
            s[p + "qkv.weight"] = (3 * t.hidden, t.hidden)  # query | key | value
            s[p + "qkv.bias"] = (3 * t.hidden,)
            s[p + "dense.weight"] = (t.hidden, t.hidden)    # attention.output.dense
            s[p + "dense.bias"] = (t.hidden,)
            s[p + "ln1.weight"] = (t.hidden,)               # attention.output.LayerNorm
            s[p + "ln1.bias"] = (t.hidden,)
            s[p + "fc1.weight"] = (t.ffn, t.hidden)         # intermediate.dense
            s[p + "fc1.bias"] = (t.ffn,)
            s[p + "fc2.weight"] = (t.hidden, t.ffn)         # output.dense
            s[p + "fc2.bias"] = (t.hidden,)
            s[p + "ln2.weight"] = (t.hidden,)               # output.LayerNorm
            s[p + "ln2.bias"] = (t.hidden,)
        s["text.mlm.dense.weight"] = (t.hidden, t.hidden)   # lm_head.dense
        s["text.mlm.dense.bias"] = (t.hidden,)
        s["text.mlm.ln.weight"] = (t.hidden,)               # lm_head.layer_norm
        s["text.mlm.ln.bias"] = (t.hidden,)
        s["text.mlm.bias"] = (t.vocab,)                     # lm_head.bias (the decoder's)
        return s
    for i in range(t.layers):
        p = f"text.layers.{i}."
        s[p + "ln1.weight"] = (t.hidden,)
        s[p + "ln1.bias"] = (t.hidden,)
        s[p + "ln2.weight"] = (t.hidden,)
        s[p + "ln2.bias"] = (t.hidden,)
        s[p + "qkv.weight"] = (3 * t.hidden, t.hidden)
        s[p + "qkv.bias"] = (3 * t.hidden,)
        s[p + "dense.weight"] = (t.hidden, t.hidden)
        s[p + "dense.bias"] = (t.hidden,)
        s[p + "fc1.weight"] = (t.ffn, t.hidden)
        s[p + "fc1.bias"] = (t.ffn,)
        s[p + "fc2.weight"] = (t.hidden, t.ffn)
        s[p + "fc2.bias"] = (t.hidden,)
    s["text.final_ln.weight"] = (t.hidden,)
    s["text.final_ln.bias"] = (t.hidden,)
    s["text.lm_head"] = (t.vocab, t.hidden)
    return s


def num_params(cfg: ModelConfig) -> int:
    n = 0
    for shape in param_shapes(cfg).values():
        k = 1
        for d in shape:
            k *= d
        n += k
    return n


def _convnext_flops(cfg: ModelConfig, executed: bool = False) -> float:
    """What FlopCounterMode (the reference's counter, src/benchmarking/flops.py) reports for one
    forward + backward of ConvNextForImageClassification, per sample.  Convolutions and Linears
    count 2·MACs forward and once more for each gradient; the stem has no input gradient (pixels
    need none).  The counter's formula for a convolution's weight gradient multiplies the output
    channels by the batch-transposed input channels, so for the depthwise conv (groups = C) it
    reports C times the MACs executed: restated here as the counter has it.  `executed`: that
    gradient at the 2·MACs it takes (the count behind `executed_mfu`).  With drop_path_rate > 0
    the whole block is still counted for every sample, as HF executes it (it computes the branch
    and multiplies by zero); the engine skips the dropped samples' block work."""
    cn = cfg.convnext
    hw = cn.side(0) ** 2
    total = 2 * 2 * hw * cn.hidden_sizes[0] * cn.channels * cn.patch ** 2
    for si, (C, depth) in enumerate(zip(cn.hidden_sizes, cn.depths)):
        hw = cn.side(si) ** 2
        if si > 0:
            total += 3 * 2 * hw * C * 4 * cn.hidden_sizes[si - 1]
        dw = 2 * hw * C * 49
        total += depth * (2 * dw + dw * (1 if executed else C) + 3 * 2 * (2 * hw * C * 4 * C))
    total += 3 * 2 * cn.hidden_sizes[-1] * cfg.num_classes
    return float(total)


def _classifier_flops(cfg: ModelConfig) -> float:
    """3 × (patch GEMM + every layer + the head's 2·hidden·num_classes): every layer is used
    and the attention is non-causal, so the executed count is the reference-convention one."""
    if cfg.convnext is not None:
        return _convnext_flops(cfg)
    v = cfg.vision
    Sv = v.num_patches + 1
    fwd = 2 * v.num_patches * v.hidden * v.channels * v.patch ** 2
    fwd += v.layers * (2 * Sv * v.hidden * (4 * v.hidden + 2 * v.ffn) + 4 * Sv * Sv * v.hidden)
    fwd += 2 * v.hidden * cfg.num_classes
    return 3.0 * fwd


def _roberta_flops(t: TextConfig, S: int) -> float:
    """3 × (layers · (2S·h·(4h + 2F) + 4S²h) + the head's dense 2S·h² + the decoder over the real
    vocabulary 2S·h·V_valid): every row is scored and the attention is square, so the executed
    count is the reference-convention one."""
    layer = 2 * S * t.hidden * (4 * t.hidden + 2 * t.ffn) + 4 * S * S * t.hidden
    return 3.0 * (t.layers * layer + 2 * S * t.hidden * t.hidden + 2 * S * t.hidden * t.n_vocab)


def _mamba_flops(t: TextConfig, S: int) -> float:
    """3 × the matmul FLOPs of the five linears of every MambaBlock (in_proj, x_proj, dt_proj,
    out_proj: 2S·(h·2I + I·(R+2N) + R·I + I·h)) plus the tied decoder over the real vocabulary.
    The convention: FlopCounterMode counts matrix multiplications only, so the conv's and the
    scan's elementwise work (in HF's torch path and in the fused kernels alike) is not counted,
    here or in the executed count — there is no attention and every row is scored, so the two
    counts are the same number."""
    I, R, N = t.d_inner, t.rank, t.d_state
    layer = 2 * S * (t.hidden * 2 * I + I * (R + 2 * N) + R * I + I * t.hidden)
    return 3.0 * (t.layers * layer + 2 * S * t.hidden * t.n_vocab)


def flops_per_sample(cfg: ModelConfig, seq_text: int) -> float:
    """Algorithmic fwd+bwd FLOPs per sample in the reference's convention
    (src/benchmarking/flops.py:9-37: FlopCounterMode over one fwd+bwd, eager
    attention counted full-square, = 3 × forward matmul FLOPs).  ViT counts all
    `layers` because the reference instantiates (and FlopCounterMode sees) them all.
    With `freeze_tower_and_llm` (llava-pretrain, src/models/llava.py:49-52) autograd runs no
    backward in the vision tower and no weight gradients in the LLM: the count is then
    vision 1× + LLM linears 2× (forward + input gradient) + attention 3× + projector 3×."""
    if cfg.classifier:
        return _classifier_flops(cfg)
    t = cfg.text
    if t.roberta:
        return _roberta_flops(t, seq_text)
    if t.mamba:
        return _mamba_flops(t, seq_text)
    S = seq_text + (cfg.vision.num_patches if cfg.vision else 0)
    if t.llama:  # q,o: h^2 each; k,v: h*kv_dim each; gate, up, down: h*F each
        kvd = t.n_kv * t.head_dim
        lin = t.layers * 2 * S * t.hidden * (2 * t.hidden + 2 * kvd + 3 * t.ffn)
        lin += 2 * S * t.hidden * t.n_vocab
    else:
        lin = t.layers * 2 * S * t.hidden * (4 * t.hidden + 2 * t.ffn)
        lin += 2 * S * t.hidden * t.vocab
    att = t.layers * 4 * S * S * t.hidden
    vis = proj = 0.0
    if cfg.vision is not None:
        v = cfg.vision
        Sv = v.num_patches + 1
        vis = 2 * v.num_patches * v.hidden * v.channels * v.patch ** 2  # (unpadded K)
        vis += v.layers * (2 * Sv * v.hidden * (4 * v.hidden + 2 * v.ffn) + 4 * Sv * Sv * v.hidden)
        proj = 2 * v.num_patches * (v.hidden * t.hidden + t.hidden * t.hidden)
    if cfg.freeze_tower_and_llm:
        return vis + 2.0 * lin + 3.0 * att + 3.0 * proj
    return 3.0 * (lin + att + vis + proj)


def executed_flops_per_sample(cfg: ModelConfig, seq_text: int) -> float:
    """The matmul FLOPs the HIP step actually executes per sample (for `executed_mfu` beside
    the reference-convention `mfu`): lm_head + CE over the scored rows only (loss-row
    compaction: the text rows but the last for LLaVA batches), causal attention counted
    over the lower triangle with the diagonal (S(S+1)/2 score/PV pairs per head instead of
    S²), and only the vision layers the model reads (`used_layers`: vision_feature_layer
    -2 leaves the last one unbuilt).  Non-causal ViT attention stays square."""
    if cfg.convnext is not None:
        return _convnext_flops(cfg, executed=True)
    if cfg.classifier:
        return _classifier_flops(cfg)
    t = cfg.text
    if t.roberta:
        return _roberta_flops(t, seq_text)
    if t.mamba:
        return _mamba_flops(t, seq_text)
    n_img = cfg.vision.num_patches if cfg.vision else 0
    S = seq_text + n_img
    scored = seq_text - 1 if cfg.vision else S  # text-only batches keep every row (<5% unscored)
    head_v = t.n_vocab if t.llama else t.vocab
    if t.llama:
        kvd = t.n_kv * t.head_dim
        lin = t.layers * 2 * S * t.hidden * (2 * t.hidden + 2 * kvd + 3 * t.ffn)
    else:
        lin = t.layers * 2 * S * t.hidden * (4 * t.hidden + 2 * t.ffn)
    lin += 2 * scored * t.hidden * head_v
    att = t.layers * 4 * (S * (S + 1) / 2) * t.hidden
    vis = proj = 0.0
    if cfg.vision is not None:
        v = cfg.vision
        Sv = v.num_patches + 1
        vis = 2 * v.num_patches * v.hidden * v.channels * v.patch ** 2
        vis += v.used_layers * (2 * Sv * v.hidden * (4 * v.hidden + 2 * v.ffn) + 4 * Sv * Sv * v.hidden)
        proj = 2 * v.num_patches * (v.hidden * t.hidden + t.hidden * t.hidden)
    if cfg.freeze_tower_and_llm:
        return vis + 2.0 * lin + 3.0 * att + 3.0 * proj
    return 3.0 * (lin + att + vis + proj)
