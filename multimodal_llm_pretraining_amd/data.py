"""Synthetic datasets of the benchmark (§8(a) row a15), restating
src/benchmarking/data.py:8-21 (text), :24-42 (image classification) and :45-77 (multimodal).

Differences, both deliberate and documented in DESIGN.md:
* samples are generated lazily and deterministically per index from (seed, index)
  instead of materialising all of them up front (the reference's 20,000 fp32 images
  at 224² are 12 GB of host RAM); distributions are the reference's: ids ~ U{0..V-1},
  pixels ~ U[0,1), attention_mask = 1, labels = ids;
* the multimodal set pre-expands the image placeholder to `image_tokens` slots (196
  for ViT-B/16 at 224²) with label -100 on those slots — the transformers-4.47 LLaVA
  expansion the build restates; text ids then avoid the image token.
  With image_tokens=1 the reference layout (one <image> token, labels = ids) is kept.

Variable-length text (`min_text_length`, default None = the fixed-length samples above,
unchanged): the number of text tokens of sample `index` is drawn from
U{min_text_length..full} by a generator of its own seeded from (seed, index), and the sample
is returned at that length; `pad_collate` right-pads a list of such samples into the batch
format of the reference's LlavaCollator (src/data/llava_data.py:169-185: input_ids,
attention_mask with zeros and labels = -100 at the pads, pixel_values).  `pack_collate` places
such samples several to a row of a fixed width instead and marks the documents by `position_ids`
(the HF packing convention: a 0 starts a document), which engine.Batch keeps apart.
"""

from __future__ import annotations

import torch
from torch.utils.data import Dataset


def _gen(seed: int, index: int) -> torch.Generator:
    return torch.Generator().manual_seed((seed * 1_000_003 + index) & 0x7FFF_FFFF_FFFF_FFFF)


def _text_len(seed: int, index: int, lo: int | None, hi: int) -> int:
    """Text tokens of sample `index`: hi, or U{lo..hi} from a generator of its own (the
    sample's ids stay a prefix of the fixed-length sample's)."""
    if lo is None:
        return hi
    return int(torch.randint(lo, hi + 1, (1,), generator=_gen(seed ^ 0x5EED_1E45, index)))


def pad_collate(samples: list[dict], pad_token_id: int = 0) -> dict:
    """Right-pad samples of unequal length to the longest: input_ids (pad_token_id at the
    pads), attention_mask (1 / 0), labels (-100 at the pads) and, when the samples carry
    them, stacked pixel_values."""
    width = max(s["input_ids"].numel() for s in samples)
    n = len(samples)
    ids = torch.full((n, width), pad_token_id, dtype=torch.int64)
    labels = torch.full((n, width), -100, dtype=torch.int64)
    mask = torch.zeros((n, width), dtype=torch.int64)
    for i, s in enumerate(samples):
        k = s["input_ids"].numel()
        ids[i, :k] = s["input_ids"]
        labels[i, :k] = s["labels"]
        mask[i, :k] = 1
    out = {"input_ids": ids, "attention_mask": mask, "labels": labels}
    if "pixel_values" in samples[0]:
        out["pixel_values"] = torch.stack([s["pixel_values"] for s in samples])
    return out


def pack_collate(samples: list[dict], width: int, pad_token_id: int = 0) -> dict:
    """Pack samples of unequal length into rows of `width` tokens: the samples are taken in
    order and each goes into the first row that still has room for it (first fit; a new row when
    none has).  Returns input_ids (pad_token_id at the trailing pads), labels (-100 at the pads),
    position_ids (each sample counts from 0; 0 at the pads) and attention_mask (1 / 0).  A sample
    longer than `width` raises ValueError.  Pairs with
    DummyTextModelingDataset(min_text_length=...)."""
    rows: list[list[dict]] = []
    used: list[int] = []
    for i, s in enumerate(samples):
        k = s["input_ids"].numel()
        if k > width:
            raise ValueError(f"pack_collate: sample {i} has {k} tokens, more than the row width "
                             f"{width}")
        if k == 0:
            raise ValueError(f"pack_collate: sample {i} is empty")
        r = next((j for j, u in enumerate(used) if u + k <= width), len(rows))
        if r == len(rows):
            rows.append([])
            used.append(0)
        rows[r].append(s)
        used[r] += k
    n = len(rows)
    ids = torch.full((n, width), pad_token_id, dtype=torch.int64)
    labels = torch.full((n, width), -100, dtype=torch.int64)
    pos = torch.zeros((n, width), dtype=torch.int64)
    mask = torch.zeros((n, width), dtype=torch.int64)
    for r, row in enumerate(rows):
        c = 0
        for s in row:
            k = s["input_ids"].numel()
            ids[r, c:c + k] = s["input_ids"]
            labels[r, c:c + k] = s["labels"]
            pos[r, c:c + k] = torch.arange(k)
            mask[r, c:c + k] = 1
            c += k
    return {"input_ids": ids, "labels": labels, "position_ids": pos, "attention_mask": mask}


class DummyTextModelingDataset(Dataset):
    def __init__(self, vocab_size: int, sequence_length: int, num_samples: int = 50_000,
                 seed: int = 0, min_text_length: int | None = None) -> None:
        super().__init__()
        if min_text_length is not None and not 1 <= min_text_length <= sequence_length:
            raise ValueError("need 1 <= min_text_length <= sequence_length")
        self.vocab_size, self.sequence_length = vocab_size, sequence_length
        self.num_samples, self.seed = num_samples, seed
        self.min_text_length = min_text_length

    def __len__(self):
        return self.num_samples

    def __getitem__(self, index):
        if not 0 <= index < self.num_samples:
            raise IndexError(index)
        ids = torch.randint(0, self.vocab_size, (self.sequence_length,), generator=_gen(self.seed, index))
        ids = ids[:_text_len(self.seed, index, self.min_text_length, self.sequence_length)]
        return {"input_ids": ids, "labels": ids.clone()}


class DummyImageClassificationDataset(Dataset):
    """src/benchmarking/data.py:24-42: pixels ~ U[0,1) [3, S, S], one label ~ U{0..C-1} per
    image — generated per index from (seed, index), not as one [N, 3, S, S] tensor."""

    def __init__(self, image_size: int, num_classes: int, num_samples: int = 20_000,
                 seed: int = 0) -> None:
        super().__init__()
        if image_size < 1 or num_classes < 1:
            raise ValueError("need image_size >= 1 and num_classes >= 1")
        self.image_size, self.num_classes = image_size, num_classes
        self.num_samples, self.seed = num_samples, seed

    def __len__(self):
        return self.num_samples

    def __getitem__(self, index):
        if not 0 <= index < self.num_samples:
            raise IndexError(index)
        g = _gen(self.seed, index)
        pixels = torch.rand((3, self.image_size, self.image_size), generator=g)
        label = torch.randint(0, self.num_classes, (), generator=g)
        return {"pixel_values": pixels, "labels": label}


class DummyMultimodalLanguageModelingDataset(Dataset):
    def __init__(self, vocab_size: int, sequence_length: int, image_size: int,
                 num_samples: int = 20_000, image_token_id: int = 32000, image_tokens: int = 1,
                 seed: int = 0, min_text_length: int | None = None) -> None:
        super().__init__()
        if not 1 <= image_tokens < sequence_length:
            raise ValueError("need 1 <= image_tokens < sequence_length")
        if min_text_length is not None and \
                not 1 <= min_text_length <= sequence_length - image_tokens:
            raise ValueError("need 1 <= min_text_length <= sequence_length - image_tokens")
        self.min_text_length = min_text_length
        self.vocab_size, self.sequence_length, self.image_size = vocab_size, sequence_length, image_size
        self.num_samples, self.image_token_id, self.image_tokens = num_samples, image_token_id, image_tokens
        self.seed = seed

    def __len__(self):
        return self.num_samples

    def __getitem__(self, index):
        if not 0 <= index < self.num_samples:
            raise IndexError(index)
        g = _gen(self.seed, index)
        n_text = self.sequence_length - self.image_tokens
        if self.image_tokens == 1:  # reference layout
            text = torch.randint(0, self.vocab_size, (n_text,), generator=g)
        else:  # U{0..V-1} \ {image_token_id}
            text = torch.randint(0, self.vocab_size - 1, (n_text,), generator=g)
            text = text + (text >= self.image_token_id).long()
        text = text[:_text_len(self.seed, index, self.min_text_length, n_text)]
        ids = torch.cat([torch.full((self.image_tokens,), self.image_token_id), text])
        labels = ids.clone()
        if self.image_tokens > 1:
            labels[: self.image_tokens] = -100
        pixels = torch.rand((3, self.image_size, self.image_size), generator=g)
        return {"attention_mask": torch.ones_like(ids), "pixel_values": pixels,
                "input_ids": ids, "labels": labels}


class PrefetchLoader:
    """The data-loader side of the step (what `trainer.get_train_dataloader()` feeds
    `benchmark_acc_optim_times`, src/benchmarking/step_time.py:49-56): micro-batches of
    `batch_size` samples of `dataset`, indices strided over the data-parallel ranks
    (DistributedSampler order without shuffling), collated and pinned by a background
    thread `depth` batches ahead — torch's CPU ops release the GIL, so generating the next
    batch overlaps the step like DataLoader workers do.  Iterates forever (wrapping the
    index range): the benchmark asks for as many batches as it times."""

    def __init__(self, dataset, batch_size: int, rank: int = 0, world: int = 1, depth: int = 2,
                 pin: bool = True):
        import queue
        import threading

        self.ds, self.bs, self.rank, self.world, self.pin = dataset, batch_size, rank, world, pin
        self.q: queue.Queue = queue.Queue(maxsize=max(1, depth))
        self._stop = threading.Event()
        self._next = 0
        self.thread = threading.Thread(target=self._run, name="mmpt-loader", daemon=True)
        self.thread.start()

    def _batch(self) -> dict:
        n = len(self.ds)
        idx = [((self._next + i) * self.world + self.rank) % n for i in range(self.bs)]
        self._next += self.bs
        samples = [self.ds[i] for i in idx]
        if "input_ids" in samples[0] and \
                len({s["input_ids"].numel() for s in samples}) > 1:  # variable-length samples
            out = pad_collate(samples)
        else:
            out = {k: torch.stack([s[k] for s in samples]) for k in samples[0]}
        if self.pin and torch.cuda.is_available():
            out = {k: t.pin_memory() for k, t in out.items()}
        return out

    def _run(self) -> None:
        try:
            while not self._stop.is_set():
                b = self._batch()
                while not self._stop.is_set():
                    try:
                        self.q.put(b, timeout=0.1)
                        break
                    except Exception:  # queue.Full
                        continue
        except BaseException as e:  # surfaced by __next__
            self.q.put(e)

    def __iter__(self):
        return self

    def __next__(self) -> dict:
        b = self.q.get()
        if isinstance(b, BaseException):
            raise RuntimeError("data loader thread failed") from b
        return b

    def close(self) -> None:
        self._stop.set()
        self.thread.join(timeout=5)
