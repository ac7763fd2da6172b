"""Packed documents on the GPU: `position_ids` through MMPTForPretraining, the engine and the
trainer, batch against singles (the method of tests/test_varlen_gpu.py): the packed batch against
its documents run one at a time through the dense path (B = 1), gradients accumulated, the same
denominator.

Tolerance: twice the discrepancy the DENSE path of the parent commit shows between a dense [4, 20]
batch (the same 80 token ids cut into four rows, no mask) and its four single-row runs — pure
summation-order noise of bf16 weight gradients summed over another set of rows, in code this
change does not touch.  Measured on an MI355X at the parent commit with `dense_noise` below (the
kernels have no atomics, so the figures reproduce): the worst per-parameter relative L2 error of
the gradient, and the relative loss difference."""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

dev = "cuda"
DENSE_NOISE = {
    "tiny-lm": (2.3523e-3, 3.8278e-8),
    "tiny-lm-d80": (2.4754e-3, 9.4565e-8),
    "tiny-llama": (2.3521e-3, 9.3767e-8),
    "tiny-mamba": (2.4910e-3, 3.2311e-8),
}
MODELS = list(DENSE_NOISE)
# The loss is one fp32 scalar, so its discrepancy is a whole number of fp32 roundings and a
# model's own dense figure can be 0 by luck of the draw: the loss bound is twice the WORST dense
# figure of the four models, for every model; the gradient bound stays per model.
LOSS_NOISE = max(v[1] for v in DENSE_NOISE.values())
S = 40
ROWS = [[22, 18], [37, 3]]  # documents per row
PADDED = [[35, 2]]          # ... and 3 trailing pads


def tolerances(name):
    return 2 * DENSE_NOISE[name][0], 2 * LOSS_NOISE


def config_of(name):
    from multimodal_llm_pretraining_amd import config as C

    if name == "tiny-lm-hdrop":  # attention dropout and hidden dropout 0.1
        return C.with_dropout(C.get_config("tiny-lm-adrop"), text=0.1, text_attention=0.1)
    return C.get_config(name)


def packed_batch(name, rows=ROWS, seed=0):
    """ids from a seed, labels = ids, position_ids restarting at every document, the mask of the
    trailing pads; `docs`: (row, first column, length) of every document, row-major."""
    cfg = config_of(name)
    g = torch.Generator().manual_seed(seed)
    B = len(rows)
    ids = torch.randint(0, cfg.text.n_vocab, (B, S), generator=g)
    pos = torch.zeros((B, S), dtype=torch.int64)
    mask = torch.zeros((B, S), dtype=torch.int64)
    docs = []
    for b, row in enumerate(rows):
        c = 0
        for n in row:
            pos[b, c:c + n] = torch.arange(n)
            docs.append((b, c, n))
            c += n
        mask[b, :c] = 1
    denom = sum(n - 1 for _, _, n in docs)
    return dict(cfg=cfg, ids=ids, labels=ids.clone(), pos=pos, mask=mask, docs=docs, denom=denom)


def run_model(model, ids, labels, denom, **kw):
    """One forward + backward that ACCUMULATES into the flat gradient buffer; returns the loss
    (the fp32 scalar as a python float)."""
    loss = model(input_ids=ids, labels=labels, num_items_in_batch=denom, **kw).loss
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().double().item()


def singles(model, mb):
    """The documents one at a time through the dense path (B = 1, no mask, no position_ids),
    gradients accumulated, the batch's denominator."""
    model.store.zero_grad()
    total = 0.0
    for b, c, n in mb["docs"]:
        total += run_model(model, mb["ids"][b:b + 1, c:c + n], mb["labels"][b:b + 1, c:c + n],
                           mb["denom"])
    return total, model.store.grad.clone()


def grad_errors(model, got, ref):
    """Worst per-parameter relative L2 error over the trainable parameters with a gradient."""
    worst, where = 0.0, None
    for n in model.store.names():
        o, k = model.store.offsets[n], model.store.g(n).numel()
        a, b = got[o:o + k].double(), ref[o:o + k].double()
        if float(b.norm()) == 0.0:
            assert float(a.norm()) == 0.0, n
            continue
        e = float((a - b).norm() / b.norm())
        if e > worst:
            worst, where = e, n
    return worst, where


def dense_noise(name):
    """The yardstick: the 80 ids of packed_batch as a dense [4, 20] batch (no mask, no
    position_ids) against its four single-row runs, on the dense path only."""
    from multimodal_llm_pretraining_amd.models import MMPTForPretraining

    mb = packed_batch(name)
    ids = mb["ids"].view(4, 20)
    mb = dict(mb, ids=ids, labels=ids.clone(), docs=[(b, 0, 20) for b in range(4)], denom=4 * 19)
    model = MMPTForPretraining(mb["cfg"], dev, seed=0)
    model.store.zero_grad()
    loss = run_model(model, mb["ids"], mb["labels"], mb["denom"])
    g = model.store.grad.clone()
    loss1, g1 = singles(model, mb)
    return grad_errors(model, g, g1)[0], abs(loss - loss1) / abs(loss1)


def packed_run(model, mb, masked=False, **over):
    model.store.zero_grad()
    model.engine.dropout_step = 0  # (dropout configs: every run draws the first step's masks)
    kw = dict(position_ids=mb["pos"])
    if masked:
        kw["attention_mask"] = mb["mask"]
    kw.update(over)
    ids, labels = kw.pop("ids", mb["ids"]), kw.pop("labels", mb["labels"])
    loss = run_model(model, ids, labels, mb["denom"], **kw)
    return loss, model.store.grad.clone()


@pytest.fixture(scope="module")
def runs():
    """Per (model, rows): the module, the batch, the packed run and the single-document reference —
    computed once, shared by the tests below and left unchanged."""
    from multimodal_llm_pretraining_amd.models import MMPTForPretraining

    cache = {}

    def get(name, padded=False):
        if (name, padded) not in cache:
            mb = packed_batch(name, PADDED if padded else ROWS)
            model = MMPTForPretraining(mb["cfg"], dev, seed=0)
            loss1, g1 = singles(model, mb)
            loss, g = packed_run(model, mb, masked=padded)
            cache[name, padded] = dict(model=model, mb=mb, loss=loss, grad=g, loss1=loss1, grad1=g1)
        return cache[name, padded]

    return get


def check_against_singles(r, name, what):
    gtol, ltol = tolerances(name)
    gerr, where = grad_errors(r["model"], r["grad"], r["grad1"])
    lerr = abs(r["loss"] - r["loss1"]) / abs(r["loss1"])
    print(f"{name} {what}: grad err {gerr:.3e} ({where}) tol {gtol:.3e}; loss err {lerr:.3e} "
          f"tol {ltol:.3e}")
    assert math.isfinite(r["loss"]) and gerr <= gtol and lerr <= ltol


@pytest.mark.parametrize("name", MODELS)
def test_packed_batch_matches_single_documents(runs, name):
    """Loss and every parameter gradient of the packed batch (rows [[22, 18], [37, 3]] at S = 40)
    equal the accumulated result of its four documents run alone through the dense path, within
    2x the dense path's own batch-against-singles discrepancy.  Measured on an MI355X (worst
    per-parameter relative L2 gradient error / relative loss error), dense [4, 20] against singles
    at the parent commit -> the packed batch against singles here:
      tiny-lm      2.352e-3 / 3.83e-8  -> 2.352e-3 / 2.39e-9
      tiny-lm-d80  2.475e-3 / 9.46e-8  -> 2.444e-3 / 4.75e-9
      tiny-llama   2.352e-3 / 9.38e-8  -> 2.382e-3 / 7.98e-8
      tiny-mamba   2.491e-3 / 3.23e-8  -> 2.391e-3 / 4.22e-8
    (bounds: 2x the model's own gradient figure; 2x the worst loss figure, see LOSS_NOISE)."""
    r = runs(name)
    assert r["model"].engine is not None
    check_against_singles(r, name, "packed")


def test_packed_and_padded_row(runs):
    """tiny-lm, row [[35, 2] + 3 pads] with attention_mask zeros: the same bounds; other pad ids,
    other labels and other position_ids under the pads change no bit.  Measured: 2.580e-3 / 2.16e-8
    against tiny-lm's dense 2.352e-3 / 3.83e-8."""
    r = runs("tiny-lm", padded=True)
    check_against_singles(r, "tiny-lm", "packed + padded")
    mb, model = r["mb"], r["model"]
    pad = mb["mask"] == 0
    ids = torch.where(pad, torch.full_like(mb["ids"], 5), mb["ids"])
    labels = torch.where(pad, torch.full_like(mb["ids"], 9), mb["labels"])
    pos = torch.where(pad, torch.full_like(mb["pos"], 7), mb["pos"])
    loss, g = packed_run(model, mb, masked=True, ids=ids, labels=labels, position_ids=pos)
    assert loss == r["loss"] and torch.equal(g, r["grad"])


@pytest.mark.parametrize("name", ["tiny-lm", "tiny-mamba", "tiny-lm-hdrop"])
def test_packed_batch_with_checkpointing(runs, name):
    """gradient_checkpointing_enable(): the recompute runs the same kernels on the same inputs —
    and redraws the same dropout masks, over more sequences than rows — so loss and gradients
    are bitwise the non-checkpointed packed run's."""
    from multimodal_llm_pretraining_amd.models import MMPTForPretraining

    if name in MODELS:
        r = runs(name)
        model, mb, loss, grad = r["model"], r["mb"], r["loss"], r["grad"]
    else:
        mb = packed_batch(name)
        assert mb["cfg"].text.hidden_dropout == 0.1 and mb["cfg"].text.attn_dropout == 0.1
        model = MMPTForPretraining(mb["cfg"], dev, seed=0)
        loss, grad = packed_run(model, mb)
        plain = MMPTForPretraining(config_of("tiny-lm"), dev, seed=0)
        assert packed_run(plain, mb)[0] != loss  # the masks are on
    model.gradient_checkpointing_enable()
    try:
        loss2, grad2 = packed_run(model, mb)
    finally:
        model.gradient_checkpointing_disable()
    assert loss2 == loss and torch.equal(grad2, grad)


@pytest.mark.parametrize("name", MODELS)
def test_arange_position_ids_change_no_bit(name):
    from multimodal_llm_pretraining_amd.models import MMPTForPretraining

    mb = packed_batch(name)
    model = MMPTForPretraining(mb["cfg"], dev, seed=0)
    model.store.zero_grad()
    base = run_model(model, mb["ids"], mb["labels"], mb["denom"])
    g = model.store.grad.clone()
    loss, g2 = packed_run(model, mb, position_ids=torch.arange(S).repeat(2, 1))
    assert loss == base and torch.equal(g2, g)


def test_trainer_step_on_a_pack_collate_batch():
    """One ManualTrainer step for tiny-mamba on what pack_collate yields."""
    from multimodal_llm_pretraining_amd.data import DummyTextModelingDataset, pack_collate
    from multimodal_llm_pretraining_amd.optim import AdamConfig
    from multimodal_llm_pretraining_amd.trainer import ManualTrainer, StepConfig

    tr = ManualTrainer(StepConfig(model="tiny-mamba", scheduler="constant"), AdamConfig(lr=1e-3), dev)
    ds = DummyTextModelingDataset(tr.cfg.text.n_vocab, S, num_samples=16, seed=3, min_text_length=2)
    samples = [ds[i] for i in range(6)]
    lens = [s["input_ids"].numel() for s in samples]
    batch = pack_collate(samples, S)
    assert batch["input_ids"].shape[0] < len(samples)  # several documents share a row
    p0 = tr.store.master.clone()
    padded = tr.stage(batch)
    assert padded.T == sum(lens) and padded.n_seq == len(lens)
    assert padded.scan_tables is not None and padded.num_items == sum(n - 1 for n in lens)
    loss = tr.train_step([padded], padded.num_items).item()
    torch.cuda.synchronize()
    assert math.isfinite(loss) and loss > 0
    assert not torch.equal(tr.store.master, p0) and torch.isfinite(tr.store.master).all()


@pytest.mark.parametrize("name", ["tiny-lm", "tiny-mamba"])
def test_module_matches_the_engine(runs, name):
    """MMPTForPretraining(position_ids=...) against the engine run directly on the same Batch;
    the parameters' .grad are views of the flat gradient buffer (as in test_dropin_module)."""
    from multimodal_llm_pretraining_amd.engine import Batch

    r = runs(name)
    model, mb = r["model"], r["mb"]
    for n, p in model.named_parameters():
        assert p.grad is not None and p.grad.data_ptr() == model.store.g(n).data_ptr(), n
    batch = Batch(mb["cfg"], mb["ids"], mb["labels"], None, model.store.device,
                  position_ids=mb["pos"])
    assert batch.n_seq == 4 and batch.lens == [22, 18, 37, 3] and batch.num_items == mb["denom"]
    model.store.zero_grad()
    loss = model.engine.forward(batch, 1.0 / mb["denom"]) / mb["denom"]
    model.engine.backward(batch)
    torch.cuda.synchronize()
    assert loss.double().item() == r["loss"] and torch.equal(model.store.grad, r["grad"])
