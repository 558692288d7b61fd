"""Class-aware train loader fixtures from the REAL reference (utils/adaptive_sampling.py, utils/utils.py, utils/torch_utils.py,
managers/BaseManager.py) + its data/data.csv, under pandas 2.3.
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_class_loaders.py

What the reference keeps inside BaseManager.get_dataloaders (the oversampling growth loop, :330-339; the weighted-random weights,
:355-372) cannot be called under the harness: those STATEMENTS are read from the reference's file when this script runs and executed on
the tables here, so the recorded lists and weights are the reference's own code's.  The schedule loop (:203-213) sits inside load_data
between dataset constructions and is not recorded: tests/test_class_loaders_cpu.py pins it to hand-written known answers.
The IoU update (managers/OCRNet_Manager.py:115-117) is the one numpy expression `(1 - a) * values + a * to_numpy(iou)`, evaluated here on
the reference's t_get_mean_iou(..., calculate_mean=False)."""
import os
import sys
import textwrap
import types

import numpy as np
import pandas as pd
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ref_harness  # noqa: E402

R = ref_harness.load()
U = R.utils
out = {}


def manager_statements(first, last):
    """the statements of BaseManager.get_dataloaders from the line that starts with `first` up to (excluding) the one that starts with `last`"""
    lines = open(os.path.join(ref_harness.REF, "managers", "BaseManager.py")).read().split("\n")
    a = next(i for i, l in enumerate(lines) if l.strip().startswith(first))
    b = next(i for i in range(a, len(lines)) if lines[i].strip().startswith(last))
    return textwrap.dedent("\n".join(lines[a:b]))


# ---- (a) data/data.csv: the 36-column table, get_class_info, get_prob / get_dist, the v1 / v2 weights
csv = pd.read_csv(os.path.join(ref_harness.REF, "data", "data.csv"))
canonical = U.CLASS_NAMES[0]
table36 = csv[canonical].to_numpy().astype(np.int64)
out["table36"] = table36
ties = [int(len(table36) - len(np.unique(table36[:, c]))) for c in range(36)]
print("data.csv: %d frames; frames sharing a count with another, per column: min %d" % (len(table36), min(ties)))
WEIGHTS = manager_statements("class_abs = ", "sampler = WeightedRandomSampler")
for exp in (1, 2, 3):
    real = len([c for c in U.CLASS_INFO[exp][0] if c != 255])
    df = U.get_class_info(csv.copy(), exp)
    out["e%d_class_info" % exp] = df[list(range(real))].to_numpy().astype(np.int64)
    for mode in ("v1", "v2"):
        env = {"df": df, "real_num_classes": real, "np": np,
               "self": types.SimpleNamespace(config={"data": {"weighted_random_mode": mode}})}
        exec(WEIGHTS, env)
        assert env["weights"].dtype == np.float32
        out["e%d_weights_%s" % (exp, mode)] = env["weights"]

rng = np.random.RandomState(7)
for K in (8, 17, 25):
    vecs = [np.full(K, 0.5, 'f'), rng.rand(K).astype('f'), rng.rand(K).astype('f') ** 3]
    v = rng.rand(K).astype('f')
    v[::3] = 0
    v[1::5] = 1
    vecs.append(v)
    vecs = np.stack(vecs)
    out["k%d_iou_vectors" % K] = vecs
    for t, name in (("1/", "inv"), ("1-", "one_minus"), ("1-**2", "one_minus_sq")):
        probs, dists = [], []
        for v in vecs:
            s = U.AdaptiveBatchSampler(data_source=None, dataframe=None, iou_values=v.copy(), dist_type=t, batch_size=1, sel_size=1)
            p = s.get_prob()
            probs.append(p)
            per_bs = []
            for bs in (1, 4, 8, 10):
                s.batch_size = bs
                per_bs.append(s.get_dist(p))
            dists.append(np.stack(per_bs))
        out["k%d_prob_%s" % (K, name)] = np.stack(probs)
        out["k%d_dist_%s" % (K, name)] = np.stack(dists)          # [vector, batch size 1 / 4 / 8 / 10, K]
        assert out["k%d_prob_%s" % (K, name)].dtype == np.float32

# ---- (b) tie-free synthetic tables: adaptive batch sequences and oversampling lists
OVERSAMPLE = manager_statements("required_num = int(len(train_df.index)", "train_set = DatasetFromDF")
SEEDS, BATCHES, BATCH, SEL = (0, 1, 2), 6, 4, 5
for K, N, exp in ((8, 97, 1), (17, 61, 2), (25, 53, 3)):
    table = np.stack([rng.permutation(N) * 5 + c for c in range(K)], 1).astype(np.int64)
    for c in range(K):
        assert len(np.unique(table[:, c])) == N, "column %d has ties" % c
    out["k%d_table" % K] = table
    frame = pd.DataFrame(table, columns=list(range(K))).reset_index()      # (train_df comes out of a reset_index(): it has an 'index' column)
    ious = rng.rand(len(SEEDS), BATCHES, K).astype('f')
    ious[:, 0] = 0.5
    seqs = []
    for si, seed in enumerate(SEEDS):
        vals = np.ones(K, 'f') * .5
        s = U.AdaptiveBatchSampler(data_source=list(range(N)), dataframe=frame, iou_values=vals, dist_type="1-**2", batch_size=BATCH,
                                   sel_size=SEL)
        np.random.seed(seed)
        it = iter(s)
        seq = []
        for b in range(BATCHES):
            vals[:] = ious[si, b]                                           # the IoU vector written before batch b is drawn
            seq.append([int(i) for i in next(it)])
        seqs.append(seq)
    out["k%d_adaptive_seeds" % K] = np.array(SEEDS)
    out["k%d_adaptive_ious" % K] = ious
    out["k%d_adaptive_batches" % K] = np.array(seqs, dtype=np.int64)
    out["k%d_adaptive_params" % K] = np.array([BATCH, SEL])
    for preset in ("default", "rare"):
        class_list = U.OVERSAMPLING_PRESETS[preset][exp - 1]
        for frac in (0.2, 0.5):
            env = {"train_df": frame.copy(), "df": frame.copy(), "class_list": class_list, "pd": pd, "np": np,
                   "self": types.SimpleNamespace(config={"data": {"oversampling_frac": frac}})}
            exec(OVERSAMPLE, env)
            out["k%d_oversampled_%s_%d" % (K, preset, int(frac * 100))] = env["train_df"]["index"].to_numpy().astype(np.int64)
        out["e%d_preset_%s" % (exp, preset)] = np.array(class_list)

# ---- (c) confusion-matrix sequences: the reference's per-class IoU and the update sequences
STEPS = 4
for K, exp in ((8, 1), (17, 2), (25, 3)):
    cms = np.zeros((STEPS, K, K), dtype=np.int32)
    for t in range(STEPS):
        scale = (40, 3000, 1500, 400)[t]
        m = (rng.rand(K, K) ** 4 * scale).astype(np.int32)
        m[np.arange(K), np.arange(K)] += (rng.rand(K) * 20 * scale).astype(np.int32)
        absent = rng.choice(K, 2, replace=False)                            # classes neither predicted nor present: 0 / 0
        m[absent, :] = 0
        m[:, absent] = 0
        only_pred = (absent[0] + 1) % K                                     # predicted, never present: diagonal 0, IoU 0 / n
        m[:, only_pred] = 0
        if t == 2:
            dom = int((absent[1] + 2) % K)
            m[dom, dom] = 12000000                                          # one class holds most pixels: r + s passes 2^24
        assert 0 < int(m.sum()) < 2 ** 24
        cms[t] = m
    out["k%d_cms" % K] = cms
    ious = [U.to_numpy(U.t_get_mean_iou(torch.from_numpy(cms[t]), exp, calculate_mean=False)) for t in range(STEPS)]
    out["k%d_cm_iou" % K] = np.stack(ious)
    assert out["k%d_cm_iou" % K].dtype == np.float32 and out["k%d_cm_iou" % K].shape == (STEPS, K)
    for a, name in ((1, "1"), (0.3, "03"), (0, "0")):
        vals = np.ones(K, 'f') * .5
        seq = []
        for t in range(STEPS):
            vals[:] = (1 - a) * vals + a * ious[t]
            seq.append(vals.copy())
        out["k%d_ema_a%s" % (K, name)] = np.stack(seq)

path = os.path.join(HERE, "class_loaders.npz")
np.savez_compressed(path, **out)
print("wrote class_loaders.npz", os.path.getsize(path), "bytes,", len(out), "arrays")
