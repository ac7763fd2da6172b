"""Padded batches on the host (no GPU): `Batch(attention_mask=...)` drops the pad tokens of a
right-padded batch and builds every index over the valid tokens — checked against a
straightforward numpy restatement written here — for the text-only and the multimodal tiny
configs; malformed masks raise; the right-padding collate helper feeds Batch unchanged."""

import numpy as np
import pytest
import torch

from multimodal_llm_pretraining_amd import config as C
from multimodal_llm_pretraining_amd.data import (DummyMultimodalLanguageModelingDataset,
                                                 DummyTextModelingDataset, pad_collate)
from multimodal_llm_pretraining_amd.engine import Batch, sort_segments

CPU = torch.device("cpu")


def padded_batch(name, text_lens, width=None, seed=0, pad_id=0, junk_labels=False):
    """A right-padded batch of len(text_lens) rows.  junk_labels: real ids (not -100) left in
    the labels under the mask, which Batch must ignore."""
    cfg = C.get_config(name)
    g = torch.Generator().manual_seed(seed)
    npch = cfg.vision.num_patches if cfg.multimodal else 0
    lens = [npch + n for n in text_lens]
    W = max(lens) if width is None else width
    B = len(lens)
    ids = torch.full((B, W), pad_id, dtype=torch.int64)
    labels = torch.full((B, W), -100, dtype=torch.int64)
    mask = torch.zeros((B, W), dtype=torch.int64)
    for b, (n, L) in enumerate(zip(text_lens, lens)):
        hi = cfg.image_token_id if cfg.multimodal else cfg.text.vocab
        text = torch.randint(0, hi, (n,), generator=g)
        row = torch.cat([torch.full((npch,), cfg.image_token_id if cfg.multimodal else 0), text])
        ids[b, :L] = row
        labels[b, :L] = row
        labels[b, :npch] = -100
        mask[b, :L] = 1
    if junk_labels:
        labels = torch.where(mask == 0, torch.full_like(labels, 7), labels)
    pix = torch.rand(B, 3, cfg.vision.image, cfg.vision.image, generator=g) if cfg.multimodal \
        else None
    return cfg, ids, labels, mask, pix


def restate(cfg, ids, labels, mask):
    """numpy restatement of what Batch must hold for a right-padded batch."""
    ids, labels, m = ids.numpy(), labels.numpy().copy(), mask.numpy() != 0
    B, W = ids.shape
    labels[~m] = -100
    shifted = np.full_like(labels, -100)
    shifted[:, :-1] = labels[:, 1:]
    lens = m.sum(1)
    out = dict(lens=[int(x) for x in lens], T=int(lens.sum()), max_len=int(lens.max()),
               cu=np.concatenate(([0], np.cumsum(lens))).astype(np.int32),
               pos=np.concatenate([np.arange(n) for n in lens]).astype(np.int32),
               ids=np.concatenate([ids[b, :lens[b]] for b in range(B)]),
               labels=np.concatenate([shifted[b, :lens[b]] for b in range(B)]))
    out["num_items"] = int((out["labels"] != -100).sum())
    return out


@pytest.mark.parametrize("name,text_lens", [("tiny-lm", [9, 1, 4, 2]), ("tiny-mm", [5, 1, 3])])
@pytest.mark.parametrize("junk", [False, True])
def test_batch_drops_pads(name, text_lens, junk):
    cfg, ids, labels, mask, pix = padded_batch(name, text_lens, pad_id=3, junk_labels=junk)
    b = Batch(cfg, ids, labels, pix, CPU, attention_mask=mask)
    r = restate(cfg, ids, labels, mask)
    assert (b.B, b.S) == tuple(ids.shape)
    assert b.T == r["T"] and b.lens == r["lens"] and b.max_len == r["max_len"]
    assert b.tokens == r["T"]
    assert b.cu_seqlens.dtype == torch.int32 and b.pos.dtype == torch.int32
    assert np.array_equal(b.cu_seqlens.numpy(), r["cu"])
    assert np.array_equal(b.pos.numpy(), r["pos"])
    assert np.array_equal(b.ids.numpy(), r["ids"])
    assert np.array_equal(b.labels.numpy(), r["labels"])
    assert b.num_items == r["num_items"]
    # the last real token of every row carries no label (the shift ran in the padded layout)
    last = r["cu"][1:] - 1
    assert (b.labels.numpy()[last] == -100).all()
    # text tokens before the last one are each other's labels
    npch = cfg.vision.num_patches if cfg.multimodal else 0
    assert b.num_items == sum(n - 1 for n in text_lens) + (len(text_lens) if npch else 0)
    # loss rows / map index the compacted rows
    keep = np.flatnonzero(r["labels"] != -100)
    if b.loss_rows is not None:
        assert np.array_equal(b.loss_rows.numpy(), keep)
        assert np.array_equal(b.loss_labels.numpy(), r["labels"][keep])
        lmap = np.full(r["T"], -1)
        lmap[keep] = np.arange(keep.size)
        assert np.array_equal(b.loss_map.numpy(), lmap)
    else:
        assert keep.size >= 0.95 * r["T"] and b.loss_labels is b.labels
    # image map over the compacted rows
    if cfg.multimodal:
        im = r["ids"] == cfg.image_token_id
        assert im.sum() == len(text_lens) * npch
        assert np.array_equal(b.img_map.numpy(), np.where(im, np.cumsum(im) - 1, -1))
        rows = np.flatnonzero(~im)
    else:
        assert b.img_map is None
        rows = np.arange(r["T"])
    # embedding-backward segments over the compacted text rows
    for got, want in zip(b.segments, sort_segments(r["ids"], rows)):
        assert np.array_equal(got.numpy(), want)
    assert int(b.segments[2].max()) < r["T"]


def test_pad_ids_and_masked_labels_do_not_matter():
    cfg, ids, labels, mask, _ = padded_batch("tiny-lm", [6, 2, 4], pad_id=0)
    a = Batch(cfg, ids, labels, None, CPU, attention_mask=mask)
    ids2 = torch.where(mask == 0, torch.full_like(ids, 11), ids)
    lab2 = torch.where(mask == 0, torch.full_like(ids, 5), labels)
    b = Batch(cfg, ids2, lab2, None, CPU, attention_mask=mask)
    for k in ("ids", "labels", "cu_seqlens", "pos"):
        assert torch.equal(getattr(a, k), getattr(b, k))
    assert a.num_items == b.num_items


@pytest.mark.parametrize("name", ["tiny-lm", "tiny-mm"])
def test_all_ones_mask_is_the_dense_path(name):
    cfg, ids, labels, mask, pix = padded_batch(name, [4, 4])
    assert bool(mask.all())
    a = Batch(cfg, ids, labels, pix, CPU)
    b = Batch(cfg, ids, labels, pix, CPU, attention_mask=mask)
    for x in (a, b):
        assert x.cu_seqlens is None and x.pos is None
        assert x.T == ids.numel() and x.max_len == ids.shape[1] and x.lens == [ids.shape[1]] * 2
    for k in ("ids", "labels", "loss_rows", "loss_labels", "loss_map", "img_map"):
        u, v = getattr(a, k), getattr(b, k)
        assert (u is None and v is None) or torch.equal(u, v)
    assert a.num_items == b.num_items
    for u, v in zip(a.segments, b.segments):
        assert torch.equal(u, v)


def test_malformed_masks_raise():
    cfg, ids, labels, mask, _ = padded_batch("tiny-lm", [6, 3])
    left = mask.clone()
    left[1] = torch.tensor([0, 0, 0, 1, 1, 1])
    with pytest.raises(ValueError, match="left-padded"):
        Batch(cfg, ids, labels, None, CPU, attention_mask=left)
    holes = mask.clone()
    holes[0, 2] = 0
    with pytest.raises(ValueError, match="holes"):
        Batch(cfg, ids, labels, None, CPU, attention_mask=holes)
    empty = mask.clone()
    empty[1] = 0
    with pytest.raises(ValueError, match="empty"):
        Batch(cfg, ids, labels, None, CPU, attention_mask=empty)
    with pytest.raises(ValueError, match="shape"):
        Batch(cfg, ids, labels, None, CPU, attention_mask=mask[:, :-1])


def test_multimodal_image_count_is_checked_on_valid_tokens():
    cfg, ids, labels, mask, pix = padded_batch("tiny-mm", [4, 2])
    ids = ids.clone()
    ids[1, -1] = cfg.image_token_id  # an image token under the mask: not counted
    Batch(cfg, ids, labels, pix, CPU, attention_mask=mask)
    ids[0, -1] = cfg.image_token_id  # a valid one too many
    with pytest.raises(ValueError, match="image tokens"):
        Batch(cfg, ids, labels, pix, CPU, attention_mask=mask)


@pytest.mark.parametrize("name", ["tiny-lm", "tiny-mm"])
def test_collate_feeds_batch(name):
    cfg = C.get_config(name)
    if cfg.multimodal:
        npch = cfg.vision.num_patches
        ds = DummyMultimodalLanguageModelingDataset(cfg.image_token_id, npch + 12, cfg.vision.image,
                                                    num_samples=8, image_token_id=cfg.image_token_id,
                                                    image_tokens=npch, seed=3, min_text_length=2)
        fixed = DummyMultimodalLanguageModelingDataset(cfg.image_token_id, npch + 12,
                                                       cfg.vision.image, num_samples=8,
                                                       image_token_id=cfg.image_token_id,
                                                       image_tokens=npch, seed=3)
    else:
        npch = 0
        ds = DummyTextModelingDataset(cfg.text.vocab, 12, num_samples=8, seed=3, min_text_length=2)
        fixed = DummyTextModelingDataset(cfg.text.vocab, 12, num_samples=8, seed=3)
    samples = [ds[i] for i in range(8)]
    lens = [s["input_ids"].numel() for s in samples]
    assert all(npch + 2 <= n <= npch + 12 for n in lens) and len(set(lens)) > 1
    assert lens == [ds[i]["input_ids"].numel() for i in range(8)]  # deterministic per index
    for s, f in zip(samples, (fixed[i] for i in range(8))):  # a prefix of the fixed-length sample
        assert torch.equal(s["input_ids"], f["input_ids"][:s["input_ids"].numel()])
        assert f["input_ids"].numel() == npch + 12
    out = pad_collate(samples, pad_token_id=1)
    assert set(out) == {"input_ids", "attention_mask", "labels"} | \
        ({"pixel_values"} if cfg.multimodal else set())
    W = max(lens)
    for i, n in enumerate(lens):
        assert out["input_ids"].shape == (8, W)
        assert (out["attention_mask"][i, :n] == 1).all() and (out["attention_mask"][i, n:] == 0).all()
        assert (out["labels"][i, n:] == -100).all() and (out["input_ids"][i, n:] == 1).all()
        assert torch.equal(out["input_ids"][i, :n], samples[i]["input_ids"])
        assert torch.equal(out["labels"][i, :n], samples[i]["labels"])
    b = Batch(cfg, out["input_ids"], out["labels"], out.get("pixel_values"), CPU,
              attention_mask=out["attention_mask"])
    assert b.lens == lens and b.T == sum(lens) and b.max_len == W
    assert b.num_items == sum(n - npch - 1 for n in lens) + (8 if npch else 0)


def test_length_list_validation():
    from multimodal_llm_pretraining_amd import kernels as K

    assert K.check_seqlens([3, 1, 2]) == ([3, 1, 2], 6, 3)
    assert K.cu_seqlens_of([3, 1, 2]).tolist() == [0, 3, 4, 6]
    for bad in ([], [3, 0], [2, -1], [1.5, 2]):
        with pytest.raises(ValueError):
            K.check_seqlens(bad)
    with pytest.raises(ValueError):
        K.check_seqlens([3, 9], max_seq=8)
