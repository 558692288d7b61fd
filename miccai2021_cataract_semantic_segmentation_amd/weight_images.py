"""Weight images: everything between "a weight tensor" and "the operand a kernel reads", for the five families of split-precision routes:
  "d3"  direct 3x3 kernels (csrc/dconv3_b3.hip: three bf16 planes; h2: csrc/dconv3_f16x2.hip, two fp16 planes + a scale record)
  "p1"  pointwise kernel (csrc/pconv1.hip): (image, record) of [O, I, 1, 1] weights, forward or transposed
  "g1"  gather launches of the same kernels: the forward image, or the stride^2 parity-class images of backward-data back to back
  "h2"  head GEMM in f16x2 (csrc/igemm_f16x2.hip): (blocked fp16 planes, scale record), forward or the transposed bank's
  "b3"  bf16x3 GEMM (csrc/igemm_bf16x3.hip): three bf16 planes, planar or blocked, forward or transposed
One lookup (weight_image) hands an image to a pass; one bank per network (WeightImages) writes the images of all its layers with a few
launches per step.  The route switches (DCONV3, P1, G1, H2W_BANK, ...) live in ops and are read from there at call time."""
import collections
import ctypes

import numpy as np
import torch

from . import ops
from ._lib import ConvDesc, check, lib, ptr, stream

_D3_ENTRY = [("w", "<i8"), ("img", "<i8"), ("C", "<i4"), ("KC", "<i4"), ("NT", "<i4"), ("dg", "<i4")]     # csrc/dconv3_b3.hip: the batch record
_P1_ENTRY = [("w", "<i8"), ("img", "<i8"), ("O", "<i4"), ("I", "<i4"), ("kh", "<i4"), ("kw", "<i4"), ("t", "<i4"), ("ky0", "<i4"), ("kys", "<i4"),
             ("nky", "<i4"), ("kx0", "<i4"), ("kxs", "<i4"), ("nkx", "<i4"), ("pad", "<i4")]      # csrc/pconv1.hip: P1Entry (64 bytes)
_BATCH = {"d3": "d3", "p1": "p1", "g1": "p1"}       # the batched launch that writes a family's images
HEAD_CAP = 64       # head entries per network


def gather_desc(Cin, Cout, kh, kw, stride, pad, dil):
    """conv descriptor for the shape-independent queries of the gather launches (csrc/pconv1.hip: catseg_gconv_*)"""
    return ConvDesc(0, 0, 0, Cin, 0, 0, Cout, kh, kw, stride, pad, dil, Cin, Cout, 0, 1)


def network_layers(flat_params, convs):
    """[(family, weight, offset in floats, stride, pad, dil)] of the convolutions whose images a network's bank writes: ONE filter (square
    stride / padding / dilation, the parameter is a view into the flat buffer; the caller leaves the stem out), then the planner's geometry
    predicates say which family takes the layer"""
    layers = []
    for m in convs:
        off = flat_params.offsets.get(id(m.weight))
        if off is None or m.stride[0] != m.stride[1] or m.padding[0] != m.padding[1] or m.dilation[0] != m.dilation[1]:
            continue
        O, I, (kh, kw), st, pd, dl, groups = m.out_channels, m.in_channels, m.kernel_size, m.stride[0], m.padding[0], m.dilation[0], m.groups
        if ops.d3_layer(I, O, kh, kw, st, pd, dl, groups):
            family = "d3"
        elif groups != 1 or I % 8:
            continue
        elif ops.p1_geometry(kh, kw, st, pd, 1):
            family = "p1" if ops.p1_layer(I, O, kh, kw, st, pd, 1) and ops.p1_layer(O, I, kh, kw, st, pd, 1) else None    # (both directions)
        else:
            family = "g1" if ops.G1 and ops.g1_dgrad_layer(gather_desc(I, O, kh, kw, st, pd, dl), I, O, kh, kw, st) else None
        if family:
            layers.append((family, m.weight.data, off, st, pd, dl))
    return layers


class WeightImages:
    """the weight images of ONE network: per step one launch over the flat parameter buffer writes both directions of every direct 3x3
    layer (catseg_dconv3_prep_batch; h2: the two-plane fp16 images with their per-layer scale records, amax + image launch), one amax + one
    image launch those of every pointwise and gather layer (catseg_pconv1_prep_batch; 1 x 1: the transposed image, kh x kw / stride s: one
    image per input-pixel parity class), instead of two small launches per layer.  Head-GEMM layers enter the first time they take that
    route (weight_image).  `table`: key -> image, persistent like the buffers it slices."""

    def __init__(self, flat, layers=(), h2=None):
        """layers: [(family "d3" / "p1" / "g1", parameter tensor (a view into flat), offset in floats, stride, pad, dil)]"""
        self.flat, self.h2 = flat, ops._trunk_h2() if h2 is None else bool(h2)
        self.table, self.heads = {}, []         # heads: [(weights, transposed, planes, scale)] in the order they came
        self.layers = collections.Counter(l[0] for l in layers)
        recs, off, slices = {"d3": [], "p1": []}, {"d3": 0, "p1": 0}, []
        kc, nt = ctypes.c_int(0), ctypes.c_int(0)

        def add(batch, key, nbytes, entries):
            slices.append((batch, key, off[batch], nbytes, len(recs[batch])))
            recs[batch].extend(entries)
            off[batch] += (nbytes + 255) // 256 * 256

        for family, w, woff, stride, pad, dil in layers:
            O, I, kh, kw = w.shape
            if family == "d3":
                lib.catseg_dconv3_layout(O, ctypes.byref(kc), ctypes.byref(nt))
                nbytes = lib.catseg_dconv3_f16x2_wimg_bytes(O) if self.h2 else lib.catseg_dconv3_wimg_bytes(O)
                for dg in (0, 1):
                    add("d3", ("d3", w.data_ptr(), bool(dg), self.h2), nbytes, [(woff, off["d3"], O, kc.value, nt.value, dg)])
            elif family == "p1":
                for t in (0, 1):
                    add("p1", ("p1", w.data_ptr(), bool(t), False), lib.catseg_pconv1_wimg_bytes(I if t else O, O if t else I),
                        [(woff, off["p1"], O, I, 1, 1, t, 0, 1, 1, 0, 1, 1, 0)])
            else:
                d = gather_desc(I, O, kh, kw, stride, pad, dil)
                for bwd in (0, 1):
                    buf = np.zeros(4, dtype=_P1_ENTRY)
                    n = lib.catseg_gconv_entries(ctypes.byref(d), bwd, woff, off["p1"], buf.ctypes.data)
                    assert n >= 1
                    add("p1", ("g1", w.data_ptr(), bool(bwd), False, stride, pad, dil), lib.catseg_gconv_wimg_bytes(ctypes.byref(d), bwd),
                        [tuple(int(v) for v in buf[i]) for i in range(n)])
        self.n, self.nbytes = {"d3": len(recs["d3"]), "p1": len(recs["p1"]), "h2": 0}, off
        self._layout = (recs, slices)   # (what _allocate needs)
        self.entries, self.images, self.records = {}, {}, {}

    def _allocate(self, batch):
        """the device buffers of one batched launch, at its first use (a network that only ever runs inference never needs them).  From
        then on they live as long as the bank and are never reallocated: a captured step (graph.GraphedTrainStep) replays the launches
        that write and read them, so their addresses must not change between passes.  `table` slices them once, here."""
        (recs, slices), dev = self._layout, self.flat.device
        rec = np.array(recs[batch], dtype=_D3_ENTRY if batch == "d3" else _P1_ENTRY)
        self.entries[batch] = torch.from_numpy(rec.view(np.uint8).copy()).to(dev)
        self.images[batch] = torch.empty(self.nbytes[batch], dtype=torch.uint8, device=dev)
        if batch == "p1" or self.h2:
            self.records[batch] = torch.zeros(2 * len(rec), dtype=torch.int32, device=dev)
        for b, key, o, nbytes, k in slices:
            if b == batch:
                img = self.images[b][o:o + nbytes]
                self.table[key] = img if b == "d3" and not self.h2 else (img, self.records[b][2 * k:2 * k + 2])

    def stale(self, flat):
        """THE rebuild rule: the flat parameter buffer is another tensor, or the trunk's arithmetic changed (head entries go with the rest)"""
        return self.flat is not flat or self.h2 != ops._trunk_h2()

    def due(self, training, with_heads):
        """the families a pass that starts now refreshes up front: the trunk's only in training, under their switches; the head images
        only where the caller can write them beside other work (with_heads), otherwise they are made in front of their GEMMs"""
        on = {"d3": ops.DCONV3 and ops.PRECISION == "bf16x3", "p1": ops.P1 and ops._trunk_h2(), "h2": with_heads and ops.H2W_BANK}
        return [f for f in ("d3", "p1", "h2") if training and on[f] and self.n[f]]

    def launch(self, families):
        """(re)write the images of these families from the current parameters, on the current stream"""
        n, e, img, rec = self.n, self.entries, self.images, self.records
        for batch in ("d3", "p1"):
            if batch in families and n[batch] and batch not in img:
                self._allocate(batch)
        if "d3" in families and n["d3"]:
            if self.h2:
                check(lib.catseg_dconv3_f16x2_prep_batch(ptr(self.flat), n["d3"], ptr(e["d3"]), ptr(img["d3"]), ptr(rec["d3"]), stream()))
            else:
                check(lib.catseg_dconv3_prep_batch(ptr(self.flat), n["d3"], ptr(e["d3"]), ptr(img["d3"]), stream()))
        if "p1" in families and n["p1"]:
            check(lib.catseg_pconv1_prep_batch(ptr(self.flat), n["p1"], ptr(e["p1"]), ptr(img["p1"]), ptr(rec["p1"]), stream()))
        if "h2" in families:
            for w, transposed, planes, scale in self.heads:
                head_image_launch(w, transposed, planes, scale)

    def refresh(self, families=("d3", "p1")):
        """launch, and tell the current pass (ops.PassState.refreshed: family -> entries written) that the table holds ITS images"""
        assert ops._state.bank is self, "refresh() serves a pass of this bank's network (ops.PassState(bank))"
        self.launch(families)
        ops._state.refreshed = {f: self.n[f] for f in families}


def head_image_launch(w, transposed, planes, scale, geometry=None):
    """amax + split of one head layer's weights (OHWI, I % 16 == 0) into blocked fp16 planes"""
    O, taps, I = geometry or (w.shape[0], w.shape[2] * w.shape[3], w.shape[1])
    fn = lib.catseg_split2h_weight_t_blocked if transposed else lib.catseg_split2h_weight_blocked
    check(fn(ptr(w), O, taps, I, ptr(planes), ptr(scale), stream()))


# Weight images of the head layers (forward: blocked planes [2, taps*I/16, O, 16]; backward-data: the transposed bank's
# [2, taps*roundup(O,16)/16, I, 16]).  Each was amax + split launched in line, in front of its GEMM on the strictly serial head path (~55 us
# with the launch gaps, six times per step).  Round 6: a layer that took this route once keeps its two image buffers in its network's bank,
# and while a step is being captured into a hipGraph EngineNet._run refreshes them all on the weight-image side stream beside stem + stage 1
# (the same hand-over as the trunk's images, ops.images_ready); everywhere else the images are made in line as before.
def _head_image(w, transposed, geometry):
    st = ops._state
    bank = st.bank if geometry is None else None        # (explicit geometry: w is a folded buffer, no parameter a bank could key)
    key = ("h2", w.data_ptr(), tuple(w.shape), transposed)
    e = bank.table.get(key) if bank is not None else None
    if e is not None and e[2] < st.refreshed.get("h2", 0):      # written by this pass's refresh (an entry that came later was not)
        ops.images_ready()
        return e[0], e[1]
    if e is None:
        O, taps, I = geometry or (w.shape[0], w.shape[2] * w.shape[3], w.shape[1])
        rows = taps * ((O + 15) // 16) if transposed else taps * I // 16
        e = (torch.empty((2, rows, I if transposed else O, 16), dtype=torch.int16, device=w.device),
             torch.empty(2, dtype=torch.int32, device=w.device), bank.n["h2"] if bank is not None else 0)
        if (bank is not None and ops.H2W_BANK and bank.n["h2"] < HEAD_CAP
                and w.untyped_storage().data_ptr() == bank.flat.untyped_storage().data_ptr()):
            bank.table[key] = e
            bank.heads.append((w, transposed, e[0], e[1]))
            bank.n["h2"] += 1
    head_image_launch(w, transposed, e[0], e[1], geometry)
    return e[0], e[1]


def _b3_image(w, transposed, blocked, geometry):
    """three bf16 planes of OHWI weights: planar [3, O, taps*I] (I % 8 == 0) / transposed [3, I, taps, roundup(O, 8)], or blocked
    [3, taps*I/16, O, 16] (I % 16 == 0) / the transposed bank's [3, taps*roundup(O,16)/16, I, 16]; never cached"""
    O, taps, I = geometry or (w.shape[0], w.shape[2] * w.shape[3], w.shape[1])
    if blocked:
        shape = (3, taps * ((O + 15) // 16), I, 16) if transposed else (3, taps * I // 16, O, 16)
        fn, args = lib.catseg_split3_weight_t_blocked if transposed else lib.catseg_split3_weight_blocked, (O, taps, I)
    elif transposed:
        shape, fn, args = (3, I, taps, (O + 7) // 8 * 8), lib.catseg_split3_weight_t, (O, taps, I)
    else:
        shape, fn, args = (3, O, taps * I), lib.catseg_split3, (taps * I, O, taps * I)
    planes = torch.empty(shape, dtype=torch.int16, device=w.device)
    check(fn(ptr(w), *args, ptr(planes), stream()))
    return planes


def weight_image(w, family, backward_data=False, h2=False, blocked=False, stride=1, pad=0, dil=1, geometry=None):
    """THE lookup: the image of weights w for a kernel of `family`, forward or backward-data (p1 / h2 / b3: the transposed image).
    h2 (d3): the two-plane fp16 image and its scale record, (image, record); blocked (b3): the blocked planes; stride, pad, dil: g1;
    geometry = (O, taps, I) where w is not a 4-D [O, I, kh, kw] tensor (conv_fwd_fused: the flat buffer catseg_fold_bn writes).
    d3 / p1 / g1: the bank's image if this pass refreshed it, else one made in line and kept in the pass.  h2: the bank's image if this pass
    refreshed it, else made in line -- into the bank's buffers where the layer has or gets an entry.  b3: made in line, every time."""
    if family == "b3":
        return _b3_image(w, backward_data, blocked, geometry)
    if family == "h2":
        return _head_image(w, bool(backward_data), geometry)
    ops.images_ready()
    st = ops._state
    key = (family, w.data_ptr(), bool(backward_data), bool(h2)) + ((stride, pad, dil) if family == "g1" else ())
    img = st.bank.table.get(key) if _BATCH[family] in st.refreshed else None
    if img is None:
        img = st.inline.get(key)
    if img is None:
        if family == "d3" and not h2:
            C = w.shape[0]
            img = st.inline[key] = torch.empty(lib.catseg_dconv3_wimg_bytes(C), dtype=torch.uint8, device=w.device)
            check(lib.catseg_dconv3_prep(ptr(w), C, 1 if backward_data else 0, ptr(img), stream()))
        else:
            # a one-layer bank over the weight tensor itself.  Nothing has to keep it alive: the image and record slices in the pass's
            # dict hold its buffers, and its entries tensor is read by the launches below only -- the caching allocator hands the
            # freed block to later work of the launching stream alone, which is ordered behind them.
            one = WeightImages(w, [(family, w, 0, stride, pad, dil)], h2=True)
            one.launch((_BATCH[family],))
            st.inline.update(one.table)
            img = st.inline[key]
    return img
