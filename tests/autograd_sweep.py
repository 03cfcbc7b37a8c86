"""The autograd contract of the training path: what a trainer does with the modules beyond one forward and one backward
with every leaf requiring grad (run by tests/test_gpu_autograd_sweep.py, coverage and premises pinned on CPU by
tests/test_autograd_cells.py).  A plain module, not a conftest, built like tests/shape_sweep.py / tests/attn_sweep.py and
reusing their inputs, modules and bounds.

``CASES`` are the smallest shapes at which each path of the training code is still taken (generic and tuned row builder,
d sqrt_w reduced in torch, two table chunks, the src variant, the fused and the composed block, two stacked layers);
``CONTRACT`` names the cells a case is put through.  ``A`` is a case's baseline (all leaves require grad, one forward,
one backward with the seed-5 upstream gradient): it is held to float64 autograd of the oracle ON THE PERMUTATIONS THE RUN
ITSELF USED (``Recorder`` wraps ``ops.sort_tables`` / ``ops.sort_tables_src``), every other cell is held to ``A`` bit for
bit -- the same kernels run on the same inputs, and the training path is deterministic -- and to float64 where its
float64 gradient differs from ``A``'s.  Nothing here touches the GPU at import time."""
from collections import namedtuple

import torch

import attn_sweep as asw
import shape_sweep as sw
import src_attn_sweep as ssw
from attn_sweep import CANCEL, D, EPS, GRAD_PARAMS, H, K, TRAIN_ROW, TRAIN_ROW_CANCEL, TRAIN_TENSOR
from shape_sweep import ATOL, BF16_TENSOR, BWD_ROW_X, DCOORDS_ROW_X, FP32_TENSOR, ILL_WEIGHT, MAX_TABLES, RTOL, row_x

Case = namedtuple("Case", "id kind variant fused layers shape y modes")
SrcOp = namedtuple("SrcOp", "id N raw B T H D C seed")

# training modes: (module precision, train_tiles)
MODES = {"fp32": ("fp32", "fp32"), "fp32_mfma": ("fp32_mfma", "fp32"), "fp32_diff": ("fp32_diff", "fp32"),
         "bf16": ("fp32", "bf16")}
# whose bounds a mode is held to: the operator's are per tile type (tests/shape_sweep.py; fp32_diff:
# tests/test_gpu_train_diff.py), the blocks' per attn_sweep.TRAIN mode (fp32_diff: tests/test_gpu_attn_train_diff.py)
OP_BOUND = {"fp32": "fp32", "fp32_mfma": "fp32", "fp32_diff": "fp32", "bf16": "bf16"}
BLK_BOUND = {"fp32": "fp32", "fp32_mfma": "fp32_mfma", "fp32_diff": "fp32", "bf16": "bf16"}
ALL_MODES = tuple(MODES)
TWO_MODES = ("fp32", "fp32_diff")
DSW_LANES = 64       # hept_amd/autograd.py: ``if h * c <= 64`` -- d sqrt_w out of the reduction kernel, else in torch
DISPATCH_LEAVES = ("q", "k", "v", "coords", "w_rpe.weight", "attn.out_linear.weight", "attn.out_linear.bias")
OP_INPUTS = ("q", "k", "v", "coords")
OP_PARAMS = ("w_rpe.weight", "attn.out_linear.weight", "attn.out_linear.bias")
OP16 = {"q": "dq", "k": "dk", "v": "dv", "coords": "dcoords", "w_rpe.weight": "dw_rpe", "attn.out_linear.weight": "dW_out",
        "attn.out_linear.bias": "db_out", "out": "out"}      # names of shape_sweep.BF16_TENSOR
FRONT = ("norm1.weight", "norm1.bias", "w_q.weight", "w_k.weight", "w_v.weight")   # HeptPartialSumsFused's front end
FF = ("norm2.weight", "norm2.bias", "ff.0.weight", "ff.0.bias", "ff.2.weight", "ff.2.bias")
ONE_HOT_ROW = 37     # a real point inside a full block of the first cloud


def _cases():
    out = []

    def op(name, sizes, t, h, d, c, modes=TWO_MODES):
        s = sw.Shape(name, tuple(sizes), 32, t, h, d, c, 10 * len(out), True)
        other = tuple(reversed(sizes)) if len(sizes) > 1 else (sizes[0] // 2, sizes[0] // 2)
        out.append(Case(name, "op", "example", None, 1, s, s._replace(sizes=other, seed=s.seed + 1), modes))

    def blk(name, kind="blk", fused=True, layers=1, modes=TWO_MODES):
        s = asw.Shape(name, (100, 60), 32, 3, 4, 10 * len(out), True, False)
        out.append(Case(name, kind, "example", fused, layers, s, s._replace(sizes=(60, 100), seed=s.seed + 1), modes))

    op("op-generic", [100, 60], 2, 3, 5, 3)             # generic row builder
    op("op-tuned", [100, 60], 2, 8, 24, 6, ALL_MODES)   # tuned row builder
    op("op-wide", [128], 2, 16, 8, 6)                   # h * c = 96 > 64: d sqrt_w reduced in torch
    op("op-chunks", [96, 40], 9, 8, 24, 4)              # two table chunks, row buffers reused by the second
    # (219 raw points: prepare_input_src pads one cloud to the next multiple of B, 224; Y has 200 raw points in as many rows)
    s = SrcOp("op-src", 224, 219, 32, 2, 8, 24, 6, 10 * len(out))
    out.append(Case("op-src", "op", "src", None, 1, s, s._replace(raw=200, seed=s.seed + 1), TWO_MODES))
    blk("blk", modes=ALL_MODES)                         # HeptPartialSumsFused + LnFfn
    blk("blk-composed", fused=False)                    # torch norm1 / w_q / w_k / w_v around HeptPartialSums
    s = ssw.Shape("blk-src", 224, 219, 32, 2, 4, False, 10 * len(out), True)
    out.append(Case("blk-src", "blk", "src", True, 1, s, s._replace(raw=200, seed=s.seed + 1), TWO_MODES))
    blk("stack2", kind="stack", layers=2)               # AttnStack: layer 2's input is no leaf
    return out


CASES = _cases()
BY_ID = {c.id: c for c in CASES}
MODULE = {("op", "example"): "HEPTAttention", ("op", "src"): "HEPTAttention-src", ("blk", "example"): "Attn",
          ("blk", "src"): "SrcAttn", ("stack", "example"): "AttnStack"}

# the contract cells (the dispatch table, cell 8, has its own tests: it needs no baseline)
CONTRACT = ("baseline", "subsets", "repeat", "two-forwards", "twice", "upstream", "onehot", "leaf16", "checkpoint",
            "second-order")
BF16_CASES = ("op-tuned", "blk")     # where the exact cells also run on bf16 tiles
CHECKPOINT_CASES = ("op-tuned", "blk", "blk-src")


def applies(case, cell):
    if cell == "onehot":           # stated on the operator's own gradients dq, dk, dv, dcoords
        return case.kind == "op"
    if cell == "leaf16":           # (AttnStack keeps float32 between its layers: INTEGRATION.md)
        return case.kind in ("op", "blk")
    if cell == "checkpoint":
        return case.id in CHECKPOINT_CASES
    return True


def cell_modes(case, cell):
    if cell == "baseline":
        return case.modes
    if cell == "second-order":
        return TWO_MODES
    return TWO_MODES + (("bf16",) if case.id in BF16_CASES else ())


def n_points(case, which="X"):
    s = case.shape if which == "X" else case.y
    return s.N if case.variant == "src" else sw.n_points(s)


def n_chunks(case):
    return -(-case.shape.T // MAX_TABLES)


def leaf_names(case):
    """(input leaves, parameter leaves) of a case."""
    if case.kind == "op":
        return OP_INPUTS, OP_PARAMS
    if case.kind == "blk":
        return ("x", "coords"), GRAD_PARAMS
    return ("x", "coords"), tuple(f"attns.{i}.{p}" for i in range(case.layers) for p in GRAD_PARAMS)


def subsets(case):
    """Cell 1: every leaf on its own, and the subsets a trainer produces; name -> set of leaves that require grad."""
    ins, params = leaf_names(case)
    every = ins + params
    out = {f"only-{nm}": {nm} for nm in every}
    out["inputs-only"] = set(ins)
    out["params-only"] = set(params)
    out["biases-only"] = {nm for nm in params if nm.endswith(".bias")}
    if case.kind == "op":
        out["all-but-v"] = set(every) - {"v"}
    else:
        base = lambda nm: nm.split(".", 2)[2] if nm.startswith("attns.") else nm
        out["all-but-v"] = {nm for nm in every if base(nm) != "w_v.weight"}
        out["x-front-end-frozen"] = {"x"} | {nm for nm in params if base(nm) not in FRONT}
        out["operator-only-front-end-frozen"] = {"coords"} | {nm for nm in params if base(nm) == "w_rpe.weight"}
        out["ff-only"] = {nm for nm in params if base(nm) in FF}
    return out


def cells(case):
    """What a case covers: its module, variant, form, dsw branch, table chunking, and every (contract cell, mode)."""
    s = case.shape
    h, c = (s.H, s.C) if case.kind == "op" else (H, s.C)
    out = {f"module:{MODULE[(case.kind, case.variant)]}", f"variant:{case.variant}",
           "bwd-dsw-kernel" if h * c <= DSW_LANES else "bwd-dsw-torch",
           "table-chunks" if s.T > MAX_TABLES else "tables-one-chunk"}
    if case.kind == "op":
        out.add("rows-tuned" if s.H == 8 and (s.D, s.C) in sw.TUNED else "rows-generic")
    else:
        out.add("fused" if case.fused else "composed")
    for cell in CONTRACT:
        if applies(case, cell):
            out.add(f"cell:{cell}")
            for m in cell_modes(case, cell):
                out |= {f"precision:{m}", f"cell:{cell}/{m}"}
            if cell == "subsets":
                out |= {f"subset:{nm}" for nm in subsets(case)}
    return out


PARAMS = [(c.id, m, cell) for c in CASES for cell in CONTRACT if applies(c, cell) for m in cell_modes(c, cell)]

# stack2, two layers against float64: per tensor max |a - r| / max |r|, per row (row_x); bounds at twice the measured
# worst on the MI355X and never above 10x attn_sweep's single-block constant of the same name
# (measured worst over the baselines of X and Y and m(X) + m(Y), fp32 tiles: per tensor 5.13e-6 (w_rpe.weight / coords)
# and 4.98e-6 (the others), per row 1.24e-5, coords / w_rpe.weight per row 4.63e-5; precision "fp32_diff" is held to the
# same bounds, as tests/test_gpu_attn_train_diff.py holds it: measured 3.34e-6, 2.74e-6, 6.14e-6, 1.44e-5.  All below the
# single-block constants 1.7e-4, 9e-5, 6.6e-4 themselves: the second layer costs no accuracy at this size)
STACK_TENSOR = {"fp32": 1.1e-5}
STACK_ROW = {"fp32": 2.5e-5}
STACK_ROW_CANCEL = {"fp32": 9.3e-5}


# ---------------------------------------------------------------------------------------------------------------------
# inputs (CPU) and the float64 reference
# ---------------------------------------------------------------------------------------------------------------------
_inputs = {}


def inputs(case, which="X"):
    """CPU inputs of a case, scaled as the existing sweeps scale theirs; "Y": the next seed and another cloud split."""
    key = (case.id, which)
    if key not in _inputs:
        s = case.shape if which == "X" else case.y
        if case.kind == "op" and case.variant == "src":
            from hept_amd.synthetic import make_inputs_src

            inp = make_inputs_src(s.raw, block_size=s.B, n_hashes=s.T, coords_dim=s.C, num_heads=s.H, h_dim=s.D,
                                  num_regions=max(4, s.N // (2 * s.B)), seed=s.seed, qk_scale=0.3, coords_scale=0.2)
            inp = dict(inp, eta=inp["eta_idx"].float().contiguous(), phi=inp["phi_idx"].float().contiguous(),
                       regions_h=inp["regions_h"].float().contiguous())
            assert inp["q"].shape[0] == s.N == inp["coords"].shape[0]
        elif case.kind == "op":
            inp = sw.inputs(s)
        elif case.variant == "src":
            inp = ssw.inputs(s)
        else:
            inp = asw.inputs(s)
        _inputs[key] = inp
    return _inputs[key]


def layer_params(case):
    """The parameters of every layer of a block / stack (CPU, the reference's state-dict names); the X inputs' own for
    the first layer, another seeded default-initialised block for each further one."""
    p0 = inputs(case)["params"]
    return [p0] + [asw.default_params(case.shape.C, case.shape.T, case.shape.seed + 100 * i)
                   for i in range(1, case.layers)]


def pad_row(case, which="X"):
    """The first padding row of the inputs (a pad copy / a raw_size padding row), or None where there is none."""
    if case.variant == "src":
        s = case.shape if which == "X" else case.y
        return s.raw if s.raw < s.N else None
    real = inputs(case, which).get("unpad_seq")      # (the operator's inputs carry it; the one-hot cell runs on those)
    if real is None:
        return None
    pads = (~real).nonzero().flatten()
    return int(pads[0]) if len(pads) else None


def g_out(shape, seed=5):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def one_hot(shape, r):
    g = torch.zeros(shape)
    g[r] = g_out(shape[1:], seed=50 + r)
    return g


def _geo(case, inp):
    if case.variant != "src":
        return None
    return dict(raw_size=inp["raw_size"], region_indices=(inp["eta"], inp["phi"]), regions_h=inp["regions_h"])


def _ill(case, res):
    total = res["denom"].detach().sum(0).squeeze(-1)          # (H, N): every table's weight of the row
    ill = int((total < ILL_WEIGHT).any(0).sum())
    assert ill == 0, f"{case.id}: {ill} rows with total weight < {ILL_WEIGHT}: rescale the shape"


def ref64(case, which, perms, g=None, req=None):
    """float64 autograd of the oracle (``forward(..., grad=True)`` / ``attn_block`` per layer, concatenated as AttnStack
    does) on the given permutations, ``perms`` = [(qpos, kpos)] per layer, None: the oracle sorts itself.  ``g`` is the
    upstream gradient (None: seed 5), ``req`` the leaves that require grad (None: all).  Returns the output under "out"
    and every gradient under its leaf's name, plus the permutations used under "perms"."""
    import hept_oracle as ho

    inp = inputs(case, which)
    ins, params = leaf_names(case)
    req = set(ins + params) if req is None else set(req)
    perms = [(None, None)] * case.layers if perms is None else perms
    s = case.shape
    geo = _geo(case, inp)
    leaves, used = {}, []

    def leaf(nm, t):
        leaves[nm] = t.double().clone().requires_grad_(nm in req)
        return leaves[nm]

    if case.kind == "op":
        px = inputs(case)       # the module's parameters are the X inputs' whichever inputs run through it
        res = ho.forward(leaf("q", inp["q"]), leaf("k", inp["k"]), leaf("v", inp["v"]), leaf("coords", inp["coords"]),
                         inp.get("combined_shifts"), leaf("w_rpe.weight", px["w_rpe_weight"]), px["alpha"].double(),
                         leaf("attn.out_linear.weight", px["out_weight"]), leaf("attn.out_linear.bias", px["out_bias"]),
                         block_size=s.B, w_per_dist=10, q_positions=perms[0][0], k_positions=perms[0][1], keep=False,
                         grad=True, geo=geo)
        _ill(case, res)
        used.append((res["q_positions"], res["k_positions"]))
        out = res["out"]
    else:
        cur = leaf("x", inp["x"])
        coords = leaf("coords", inp["coords"])
        outs = [cur]
        for i, p in enumerate(layer_params(case)):
            pre = f"attns.{i}." if case.kind == "stack" else ""
            p64 = {k: (leaf(pre + k, v) if k in GRAD_PARAMS else v.double()) for k, v in p.items()}
            res = ho.attn_block(cur, coords, inp.get("combined_shifts"), p64, num_heads=H, block_size=s.B, w_per_dist=K,
                                eps=EPS, q_positions=perms[i][0], k_positions=perms[i][1], keep=False, grad=True,
                                **({} if geo is None else {"geo": geo}))
            _ill(case, res)
            used.append((res["q_positions"], res["k_positions"]))
            cur = res["y"]
            outs.append(cur)
        out = cur if case.kind == "blk" else torch.cat(outs, dim=-1)
    want = {"out": out.detach(), "perms": used}
    if out.requires_grad:
        out.backward((g_out(out.shape) if g is None else g).double())
    for nm, t in leaves.items():
        want[nm] = t.grad if t.grad is not None else (torch.zeros_like(t) if nm in req else None)
    return want


def one_hot_rows(perms, r, block_size):
    """Cell 5: the rows a one-hot upstream gradient in row ``r`` may reach.  dq: ``r`` alone; dk, dv: the rows
    ``kpos[t, h, block(r)]`` over all (t, h), ``block(r)`` the block of r's position in ``qpos[t, h]``; dcoords: their
    union with r.  ``perms`` = (qpos, kpos), (T, H, N) each."""
    qpos, kpos = perms[0].long(), perms[1].long()
    at = (qpos == r).long().argmax(-1)                               # (T, H): r's position in every sorted order
    cols = (at // block_size)[..., None] * block_size + torch.arange(block_size)
    keys = set(kpos.gather(-1, cols).flatten().tolist())
    return {"q": {r}, "k": keys, "v": keys, "coords": keys | {r}}


def outside(t, rows):
    """max |t| over the rows NOT in ``rows``."""
    keep = torch.ones(t.shape[0], dtype=torch.bool)
    keep[sorted(rows)] = False
    return float(t[keep].abs().max()) if bool(keep.any()) else 0.0


# ---------------------------------------------------------------------------------------------------------------------
# GPU side (imports deferred: the CPU suite imports this module without a GPU)
# ---------------------------------------------------------------------------------------------------------------------
class Recorder:
    """Wraps ``ops.sort_tables`` and ``ops.sort_tables_src`` (hept_amd/autograd.py calls them through the module, so the
    wrapper is reached) and keeps every (qpos, kpos) they return, in call order."""

    def __init__(self, monkeypatch):
        from hept_amd import ops

        self.calls = []
        for name in ("sort_tables", "sort_tables_src"):
            monkeypatch.setattr(ops, name, self._wrap(getattr(ops, name)))

    def _wrap(self, fn):
        def recorded(*a, **kw):
            qp, kp = fn(*a, **kw)
            self.calls.append((qp, kp))
            return qp, kp

        return recorded


Run = namedtuple("Run", "out grads perms")


class Rig:
    """One case's module in one training mode on the GPU, its leaves and its forward."""

    def __init__(self, case, mode, dev, rec=None, precision=None):
        import hept_amd

        self.case, self.mode, self.dev, self.rec = case, mode, dev, rec
        self.input_names, self.param_names = leaf_names(case)
        self.all = self.input_names + self.param_names
        prec, tiles = MODES[mode]
        prec = prec if precision is None else precision      # (the dispatch table also runs 16-bit inference tiles)
        s, inp = case.shape, inputs(case)
        if case.kind == "op":
            attn = hept_amd.HEPTAttention(s.D + s.C, precision=prec, variant=case.variant, h_dim=s.D, num_heads=s.H,
                                          block_size=s.B, n_hashes=s.T, num_w_per_dist=10)
            sd = {"out_linear.weight": inp["out_weight"], "out_linear.bias": inp["out_bias"], "e2lsh.alpha": inp["alpha"]}
            if case.variant == "src":
                sd["e2lsh.beta"] = torch.zeros(1, s.T)
            attn.load_state_dict(sd, strict=True)
            net = torch.nn.Module()
            net.attn = attn
            net.w_rpe = torch.nn.Linear(inp["w_rpe_weight"].shape[1], inp["w_rpe_weight"].shape[0])
            with torch.no_grad():
                net.w_rpe.weight.copy_(inp["w_rpe_weight"])
            self.ops_ = [attn]
        elif case.kind == "blk":
            net = (ssw if case.variant == "src" else asw).module(s, inp, prec, "cpu")
            net.fuse_training = case.fused
            self.blocks, self.ops_ = [net], [net.attn]
        else:
            net = hept_amd.AttnStack(s.C, precision=prec, n_layers=case.layers, h_dim=D, num_heads=H, block_size=s.B,
                                     n_hashes=s.T, num_w_per_dist=K)
            net.load_state_dict({f"attns.{i}.{k}": v for i, p in enumerate(layer_params(case)) for k, v in p.items()},
                                strict=True)
            self.blocks, self.ops_ = list(net.attns), [b.attn for b in net.attns]
        for b in getattr(self, "blocks", []):
            b.dropout.p = 0.0
        for a in self.ops_:
            a.train_tiles = tiles
        self.net = net.to(dev).train()
        self.params = dict(self.net.named_parameters())
        self.never = [p for nm, p in self.params.items() if nm not in self.param_names]   # e2lsh.alpha / beta, w_rpe.bias
        self.gpu = {}

    def data(self, which):
        if which not in self.gpu:
            inp = inputs(self.case, which)
            self.gpu[which] = {k: v.to(self.dev) for k, v in inp.items() if torch.is_tensor(v)}
            self.gpu[which]["raw_size"] = inp.get("raw_size")
        return self.gpu[which]

    def set_params(self, req=None):
        """Which parameters require grad (None: all that can); clears every .grad."""
        for nm in self.param_names:
            self.params[nm].requires_grad_(req is None or nm in req)
        for p in self.params.values():
            p.grad = None

    def make_inputs(self, which="X", req=None, dtype=None, widened=False):
        """Fresh input leaves.  ``dtype``: q, k, v / x as 16-bit leaves; ``widened``: their rounded values as float32."""
        g, out = self.data(which), {}
        for nm in self.input_names:
            t = g[nm].clone()
            if dtype is not None and nm != "coords":
                t = t.to(dtype).float() if widened else t.to(dtype)
            out[nm] = t.requires_grad_(req is None or nm in req)
        return out

    def leaves(self, which="X", req=None, dtype=None, widened=False):
        self.set_params(req)
        return self.make_inputs(which, req, dtype, widened)

    def kwargs(self, ins, which):
        g = self.data(which)
        if self.case.variant == "src":
            return {"raw_size": g["raw_size"], "coords": ins["coords"], "region_indices": [g["eta"], g["phi"]],
                    "regions_h": g["regions_h"]}
        return {"coords": ins["coords"], "combined_shifts": g["combined_shifts"]}

    def call(self, *tensors, which="X"):
        """The module on positional input tensors (what torch.utils.checkpoint passes on)."""
        ins = dict(zip(self.input_names, tensors))
        kw = self.kwargs(ins, which)
        if self.case.kind == "op":
            return self.net.attn(ins["q"], ins["k"], ins["v"], w_rpe=self.net.w_rpe, **kw)
        return self.net(ins["x"], kw)

    def forward(self, ins, which="X", count=1):
        """One forward; returns the output and the permutations it used, per layer (chunks concatenated).  A recorder
        that caught another number of sort calls than forwards x layers x ceil(T / 8) fails here."""
        n0 = len(self.rec.calls)
        out = self.call(*(ins[nm] for nm in self.input_names), which=which)
        return out, self.taken(n0, which, count)

    def taken(self, n0, which="X", count=1):
        calls = self.rec.calls[n0:]
        case, ch = self.case, n_chunks(self.case)
        assert len(calls) == count * case.layers * ch, \
            f"{case.id}: {len(calls)} recorded sort calls, expected {count} x {case.layers} x {ch}"
        perms = []
        for i in range(0, len(calls), ch):
            qp = torch.cat([c[0] for c in calls[i:i + ch]]).long().cpu()
            kp = torch.cat([c[1] for c in calls[i:i + ch]]).long().cpu()
            assert tuple(qp.shape) == (case.shape.T, len(qp[0]), n_points(case, which)) == tuple(kp.shape), case.id
            perms.append((qp, kp))
        return perms

    def grads(self, ins):
        """Every leaf's .grad on the CPU (None where there is none); alpha and w_rpe.bias must never hold one."""
        for p in self.never:
            assert p.grad is None, f"{self.case.id}: a frozen / unused parameter received a gradient"
        out = {nm: ins[nm].grad for nm in self.input_names}
        out.update({nm: self.params[nm].grad for nm in self.param_names})
        return {nm: (None if t is None else t.detach().cpu().clone()) for nm, t in out.items()}

    def operator_trains(self, req):
        """Whether the operator's training path runs: always in the fused blocks; in the composed block (and a direct
        call) only if something in or in front of the operator requires grad -- with nothing but norm2 / ff to train,
        the composed block's operator is served by its one-call inference path, which sorts inside that call."""
        if req is None or self.case.kind == "stack" or (self.case.kind == "blk" and self.case.fused):
            return True
        return any(nm.split(".", 2)[-1] not in FF and nm not in FF for nm in req)

    def step(self, which="X", req=None, g=None, dtype=None, widened=False):
        """Fresh leaves, one forward, one backward."""
        ins = self.leaves(which, req, dtype, widened)
        n0 = len(self.rec.calls)
        out = self.call(*(ins[nm] for nm in self.input_names), which=which)
        assert out.requires_grad and out.grad_fn is not None, \
            f"{self.case.id} {self.mode}: leaves {sorted(self.all if req is None else req)} require grad, the output " \
            f"carries no graph"
        perms = self.taken(n0, which, 1 if self.operator_trains(req) else 0)
        g = g_out(out.shape) if g is None else g
        out.backward(g.to(self.dev).to(out.dtype) if g.device.type == "cpu" else g)
        return Run(out.detach().cpu(), self.grads(ins), perms)


def hold64(case, mode, got, want, note, tag=""):
    """Every gradient in ``want`` (and the output) against float64, under the bounds the project already uses for the
    module and mode (``stack2``: its own, see STACK_*).  ``note(name, value)`` sees every figure before it is asserted."""
    names = [nm for nm in want if nm not in ("perms",) and want[nm] is not None]
    worst_t, worst_r = {}, {}
    for nm in names:
        a, r = got[nm], want[nm]
        assert a is not None, (case.id, mode, tag, nm)
        assert bool(torch.isfinite(a).all()), (case.id, mode, tag, nm)
        worst_t[nm] = float((a.double() - r).abs().max()) / (float(r.abs().max()) + 1e-300)
        worst_r[nm] = row_x(a, r)
    grads = [nm for nm in names if nm != "out"]
    base = lambda nm: nm.split(".", 2)[2] if nm.startswith("attns.") else nm
    if mode != "bf16" and "out" in names:
        out_x = float(((got["out"].double() - want["out"]).abs() / (ATOL + RTOL * want["out"].abs())).max())
        note(f"{tag}out x", out_x)
        assert out_x <= 1.0, f"{case.id} {mode} {tag}: training forward, worst element {out_x:.3f}x the fp32 tolerance"
    if case.kind == "op":
        tiles = OP_BOUND[mode]
        tb = {nm: (FP32_TENSOR if tiles == "fp32" else BF16_TENSOR[OP16[nm]]) for nm in names}
        rb = {nm: (DCOORDS_ROW_X if nm == "coords" else BWD_ROW_X)[tiles] for nm in grads}
        if tiles == "fp32":
            tb.pop("out", None)
    elif case.kind == "blk":
        bm = BLK_BOUND[mode]
        tb = {nm: TRAIN_TENSOR[bm] for nm in names}
        # (attn_sweep's bounds for the src block too: src_attn_sweep widens them only for a last block holding ONE real
        #  point, and blk-src's holds 27)
        rb = {nm: (TRAIN_ROW_CANCEL if nm in CANCEL else TRAIN_ROW)[bm] for nm in grads}
    else:
        bm = BLK_BOUND[mode]
        tb = {nm: STACK_TENSOR[bm] for nm in names}
        rb = {nm: (STACK_ROW_CANCEL if base(nm) in CANCEL else STACK_ROW)[bm] for nm in grads}
    for nm in names:
        kind = "cancel" if base(nm) in CANCEL else ("out" if nm == "out" else "grad")
        note(f"{tag}{kind} tensor", worst_t[nm])
        if nm != "out":
            note(f"{tag}{kind} row", worst_r[nm])
    bad = {nm: (w, tb[nm]) for nm, w in worst_t.items() if nm in tb and w > tb[nm]}
    assert not bad, f"{case.id} {mode} {tag}: per-tensor errors over the bound (error, bound): {bad}"
    rbad = {nm: (worst_r[nm], rb[nm]) for nm in grads if worst_r[nm] > rb[nm]}
    assert not rbad, f"{case.id} {mode} {tag}: per-row errors over the bound (error, bound): {rbad}"


def same(case, mode, tag, got, want, names=None):
    """Bit for bit: every leaf in ``names`` (default: all of ``want``) has the gradient of ``want``; None where None."""
    for nm in (want if names is None else names):
        a, r = got[nm], want[nm]
        if r is None:
            assert a is None, f"{case.id} {mode} {tag}: {nm} does not require grad but holds one"
            continue
        assert a is not None, f"{case.id} {mode} {tag}: {nm} requires grad and received none"
        assert a.dtype == r.dtype and torch.equal(a, r), \
            f"{case.id} {mode} {tag}: {nm} differs, max |diff| {float((a.double() - r.double()).abs().max()):.3e}"


_base = {}


class Cells:
    """The contract cells of one (case, mode); ``note(name, value)`` collects measured errors."""

    def __init__(self, case, mode, dev, monkeypatch, note=lambda k, v: None):
        self.case, self.mode, self.dev, self.note = case, mode, dev, note
        self.rec = Recorder(monkeypatch)
        self.rig = Rig(case, mode, dev, self.rec)

    def base(self, which="X"):
        """A: all leaves, one forward, one backward with the seed-5 upstream gradient; held to float64 on the run's own
        permutations.  Computed once per (case, mode, inputs) and left unchanged."""
        key = (self.case.id, self.mode, which)
        if key not in _base:
            run = self.rig.step(which)
            want = self.want(which, run.perms)
            hold64(self.case, self.mode, dict(run.grads, out=run.out), want, self.note, tag="" if which == "X" else "Y ")
            _base[key] = run
        return _base[key]

    def want(self, which, perms, g=None, tag=None):
        """float64 gradients on the given permutations (cached per (case, inputs, upstream gradient, permutations))."""
        key = (self.case.id, "ref64", which, tag)
        hit = _base.get(key)
        if hit is not None and all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(hit["perms"], perms)):
            return hit
        _base[key] = ref64(self.case, which, perms, g)
        return _base[key]

    def got(self, run):
        return dict(run.grads, out=run.out)

    # --- cell 0 / 10 -------------------------------------------------------------------------------------------------
    def baseline(self):
        self.base("X")

    # --- cell 1 ------------------------------------------------------------------------------------------------------
    def subsets(self):
        a = self.base()
        for name, req in subsets(self.case).items():
            run = self.rig.step(req=req)
            assert torch.equal(run.out, a.out), (self.case.id, self.mode, name)
            for p, q in zip(run.perms, a.perms):
                assert torch.equal(p[0], q[0]) and torch.equal(p[1], q[1]), (self.case.id, self.mode, name)
            same(self.case, self.mode, name, run.grads, {nm: (a.grads[nm] if nm in req else None) for nm in self.rig.all})

    # --- cell 2 ------------------------------------------------------------------------------------------------------
    def repeat(self):
        a, rig, dev = self.base(), self.rig, self.dev
        g = g_out(a.out.shape).to(dev)
        ins = rig.leaves()
        out, _ = rig.forward(ins)
        out.backward(g, retain_graph=True)
        out.backward(g)
        same(self.case, self.mode, "retain_graph twice", rig.grads(ins), {nm: 2 * t for nm, t in a.grads.items()})
        # accumulation into a pre-filled .grad: one add
        ins = rig.leaves()
        g0 = {nm: g_out(t.shape, seed=70 + i) for i, (nm, t) in enumerate(sorted(a.grads.items()))}
        for nm in rig.all:
            (ins[nm] if nm in ins else rig.params[nm]).grad = g0[nm].to(dev)
        out, _ = rig.forward(ins)
        out.backward(g)
        same(self.case, self.mode, "pre-filled .grad", rig.grads(ins), {nm: g0[nm] + t for nm, t in a.grads.items()})
        # torch.autograd.grad of two leaves: their gradients, every .grad untouched
        ins = rig.leaves()
        out, _ = rig.forward(ins)
        second = "k" if self.case.kind == "op" else "x"
        bias = [nm for nm in rig.param_names if nm.endswith("out_linear.bias")][-1]
        gk, gb = torch.autograd.grad(out, [ins[second], rig.params[bias]], g)
        same(self.case, self.mode, "autograd.grad", {second: gk.cpu(), bias: gb.cpu()}, a.grads, names=(second, bias))
        assert all(t is None for t in rig.grads(ins).values()), "torch.autograd.grad touched a .grad"

    # --- cell 3 ------------------------------------------------------------------------------------------------------
    def two_forwards(self):
        ax, ay, rig, dev = self.base("X"), self.base("Y"), self.rig, self.dev
        assert not torch.equal(ax.perms[0][0], ay.perms[0][0]), "X and Y sort alike: the cell would show nothing"
        g = g_out(ax.out.shape).to(dev)
        rig.set_params()
        ix, iy = rig.make_inputs("X"), rig.make_inputs("Y")
        out_x, px = rig.forward(ix, "X")
        out_y, py = rig.forward(iy, "Y")
        for (p, q) in zip(px + py, ax.perms + ay.perms):
            assert torch.equal(p[0], q[0]) and torch.equal(p[1], q[1]), "the permutations changed between runs"
        out_y.backward(g)
        same(self.case, self.mode, "Y behind X, backward first", rig.grads(iy), ay.grads)
        for p in rig.params.values():
            p.grad = None
        out_x.backward(g)
        same(self.case, self.mode, "X, backward after Y's", rig.grads(ix), ax.grads)
        # an inference forward (eval, no_grad: the module's cached workspace) between a training forward and its backward
        ins = rig.leaves()
        out, _ = rig.forward(ins)
        rig.net.eval()
        with torch.no_grad():
            for which in ("Y", "X"):
                rig.call(*(t.detach() for t in rig.make_inputs(which).values()), which=which)
        rig.net.train()
        out.backward(g)
        same(self.case, self.mode, "inference forward in between", rig.grads(ins), ax.grads)

    # --- cell 4 ------------------------------------------------------------------------------------------------------
    def twice(self):
        ax, ay, rig, dev = self.base("X"), self.base("Y"), self.rig, self.dev
        rig.set_params()
        ix, iy = rig.make_inputs("X"), rig.make_inputs("Y")
        out_x, px = rig.forward(ix, "X")
        out_y, py = rig.forward(iy, "Y")
        (out_x + out_y).backward(g_out(ax.out.shape).to(dev))
        gx, gy = rig.grads(ix), rig.grads(iy)
        same(self.case, self.mode, "m(X) + m(Y), inputs of X", gx, ax.grads, names=rig.input_names)
        same(self.case, self.mode, "m(X) + m(Y), inputs of Y", gy, ay.grads, names=rig.input_names)
        same(self.case, self.mode, "m(X) + m(Y), parameters", gx,
             {nm: ax.grads[nm] + ay.grads[nm] for nm in rig.param_names})
        wx, wy = self.want("X", px), self.want("Y", py)
        hold64(self.case, self.mode, {nm: gx[nm] for nm in rig.param_names},
               {nm: wx[nm] + wy[nm] for nm in rig.param_names}, self.note, tag="m(X)+m(Y) ")

    # --- cell 5 ------------------------------------------------------------------------------------------------------
    def upstream(self):
        a, rig, dev, case, mode = self.base(), self.rig, self.dev, self.case, self.mode
        shape = a.out.shape
        run = rig.step(g=torch.zeros(shape))
        for nm, t in run.grads.items():
            assert bool(torch.isfinite(t).all()) and float(t.abs().max()) == 0.0, f"{case.id} {mode}: g_out = 0, {nm}"
        # y.sum(): a stride-0 expanded upstream gradient, against its dense copy
        dense = rig.step(g=torch.ones(shape))
        ins = rig.leaves()
        out, _ = rig.forward(ins)
        out.sum().backward()
        # ... bit for bit, except where the expanded gradient goes straight into a torch GEMM: the composed block's last
        # layer is nn.Linear, whose weight gradient g^T.hidden torch hands to rocBLAS with the stride-0 operand as it is --
        # another GEMM kernel than for the dense copy, another summation order (measured 7.6e-6 absolute).  No kernel of
        # this project sees that operand (LnFfn and HeptCombine take g.contiguous()); those two gradients are held to
        # float64 instead, under the block's bounds
        loose = tuple(nm for nm in rig.param_names if nm.endswith(("ff.2.weight", "ff.2.bias"))) \
            if case.kind == "blk" and not case.fused else ()
        got = rig.grads(ins)
        same(case, mode, "y.sum() (stride 0)", got, dense.grads, names=[nm for nm in rig.all if nm not in loose])
        if loose:
            want = self.want("X", a.perms, torch.ones(shape), tag="ones")
            hold64(case, mode, {nm: got[nm] for nm in loose}, {nm: want[nm] for nm in loose}, self.note, tag="stride-0 ")
        # transposed storage
        g = g_out(shape).to(dev).t().contiguous().t()
        assert not g.is_contiguous()
        run = rig.step(g=g)
        if case.kind == "blk" and not case.fused:
            # the same exception, one step further: the composed block's ff.2 is nn.Linear, whose backward g.W2 and
            # g^T.hidden torch runs as rocBLAS GEMMs on the operand's own layout (TN for the transposed storage, NN for
            # the dense copy: measured 4.8e-7 absolute on x.grad), and everything behind them inherits the other
            # rounding.  The kernels of this project run on g.contiguous() as before; the cell is held to float64 here
            hold64(case, mode, self.got(run), self.want("X", a.perms), self.note, tag="transposed ")
        else:
            same(case, mode, "transposed g_out", run.grads, a.grads)
        if mode != "bf16":      # powers of two scale every float32 step exactly (bf16 tiles round the scaled values)
            for e in (-3, 5):
                run = rig.step(g=g_out(shape) * 2.0 ** e)
                same(case, mode, f"g_out * 2^{e}", run.grads, {nm: t * 2.0 ** e for nm, t in a.grads.items()})

    def onehot(self):
        rig, case, mode = self.rig, self.case, self.mode
        n = n_points(case)
        for kind, r in (("full", ONE_HOT_ROW), ("pad", pad_row(case))):
            if r is None:
                continue
            g = one_hot((n, case.shape.D), r)
            run = rig.step(g=g)
            rows = one_hot_rows(run.perms[0], r, case.shape.B)
            assert len(rows["k"]) < n, "the one-hot row reaches every row: the cell would show nothing"
            for nm, allowed in rows.items():
                worst = outside(run.grads[nm], allowed)
                assert worst == 0.0, f"{case.id} {mode} one-hot row {r} ({kind}): {nm} is {worst:.3e} outside its rows"
            hold64(case, mode, self.got(run), self.want("X", run.perms, g, tag=f"onehot-{r}"), self.note,
                   tag=f"one-hot {kind} ")

    # --- cell 6 ------------------------------------------------------------------------------------------------------
    def leaf16(self):
        rig, case, mode, dev = self.rig, self.case, self.mode, self.dev
        for dt in ((torch.bfloat16, torch.float16) if case.kind == "op" else (torch.bfloat16,)):
            g16 = g_out(self.base().out.shape).to(dt)
            wide = rig.step(dtype=dt, widened=True, g=g16.float())
            run = rig.step(dtype=dt, g=g16)
            assert run.out.dtype == dt and torch.equal(run.out, wide.out.to(dt)), (case.id, mode, dt)
            for nm in rig.all:
                leaf16 = nm in rig.input_names and nm != "coords"
                assert run.grads[nm].dtype == (dt if leaf16 else torch.float32), (case.id, mode, nm, dt)
            same(case, mode, f"{dt} leaves", run.grads,
                 {nm: (t.to(dt) if nm in rig.input_names and nm != "coords" else t) for nm, t in wide.grads.items()})

    # --- cell 7 ------------------------------------------------------------------------------------------------------
    def checkpoint(self):
        from torch.utils.checkpoint import checkpoint

        a, rig, case, mode, dev = self.base(), self.rig, self.case, self.mode, self.dev
        g = g_out(a.out.shape).to(dev)
        for reentrant in (False, True):
            ins = rig.leaves()
            n0 = len(self.rec.calls)
            out = checkpoint(rig.call, *(ins[nm] for nm in rig.input_names), use_reentrant=reentrant)
            first = out.detach().cpu()
            out.backward(g)
            # the training forward runs once in the forward (not under reentrant: no_grad, the inference path, which
            # sorts inside its one C call) and once more in the backward
            perms = rig.taken(n0, count=1 if reentrant else 2)
            for p, q in zip(perms, a.perms * 2):
                assert torch.equal(p[0], q[0]) and torch.equal(p[1], q[1])
            same(case, mode, f"checkpoint(use_reentrant={reentrant})", rig.grads(ins), a.grads)
            if reentrant:       # the inference path's output: held to float64, not to bit equality
                ref = self.want("X", a.perms)["out"]
                x = float(((first.double() - ref).abs() / (ATOL + RTOL * ref.abs())).max())
                self.note("checkpoint reentrant out x", x)
                # (the module's inference precision is an fp32 one in every training mode, bf16 training tiles included)
                assert x <= 1.0, f"{case.id} {mode}: the no_grad forward is {x:.3f}x the fp32 tolerance off float64"
            else:
                assert torch.equal(first, a.out)

    # --- cell 9 ------------------------------------------------------------------------------------------------------
    def second_order(self):
        import pytest

        rig = self.rig
        for nm in ("coords", "x") if self.case.kind != "op" else ("coords",):
            ins = rig.leaves()
            out, _ = rig.forward(ins)
            g = g_out(out.shape).to(self.dev)
            with pytest.raises(RuntimeError):
                (first,) = torch.autograd.grad(out, ins[nm], g, create_graph=True)
                wrt = [t for t in list(ins.values()) + [rig.params[p] for p in rig.param_names]]
                torch.autograd.grad(first.sum(), wrt, allow_unused=True)

    def run(self, cell):
        getattr(self, cell.replace("-", "_"))()


# ---------------------------------------------------------------------------------------------------------------------
# cell 8: the dispatch table
# ---------------------------------------------------------------------------------------------------------------------
DISPATCH_PRECISIONS = ("fp32", "fp32_diff", "bf16")
LIGHT = ("fp32", "fp32_mfma", "fp32_diff")     # hept_amd/hept.py: precisions whose eval-mode call takes the autograd path


def expect_dispatch(precision, training, grad, req):
    """(out.requires_grad, warns) of a direct HEPTAttention call.  The output carries a graph exactly when grad is enabled
    and any of the seven leaves requires grad; the single documented exception: eval mode with 16-bit tiles and no input
    gradient runs the inference path and warns (once per module)."""
    if not grad or not req:
        return False, False
    if precision not in LIGHT and not training and not (set(req) & set(OP_INPUTS)):
        return False, True
    return True, False


def check_dispatch_op(case, precision, dev):
    import warnings

    rig = Rig(case, "fp32", dev, precision=precision)
    attn = rig.net.attn
    n_checked = 0
    for training in (True, False):
        rig.net.train(training)
        for grad in (True, False):
            for mask in range(1 << len(DISPATCH_LEAVES)):
                req = {nm for i, nm in enumerate(DISPATCH_LEAVES) if mask >> i & 1}
                ins = rig.leaves(req=req)
                attn._warned_eval_grad = False
                with torch.set_grad_enabled(grad), warnings.catch_warnings(record=True) as caught:
                    warnings.simplefilter("always")
                    out = rig.call(*(ins[nm] for nm in rig.input_names))
                want, warns = expect_dispatch(precision, training, grad, req)
                what = f"{case.id} {precision} training={training} grad={grad} requires_grad={sorted(req)}"
                assert out.requires_grad == want and (out.grad_fn is not None) == want, what
                assert len(caught) == (1 if warns else 0), (what, [str(w.message) for w in caught])
                if warns:       # ... once: the same call again is silent
                    with warnings.catch_warnings(record=True) as again:
                        warnings.simplefilter("always")
                        rig.call(*(ins[nm] for nm in rig.input_names))
                    assert not again, what
                if want and (len(req) == 1 or len(req) == len(DISPATCH_LEAVES)):
                    out.sum().backward()
                    got = rig.grads(ins)     # (asserts that e2lsh.alpha and w_rpe.bias hold none)
                    assert {nm for nm, t in got.items() if t is not None} == req, what
                n_checked += 1
    rig.net.train()
    return n_checked


def check_dispatch_block(case, precision, dev, monkeypatch):
    """Attn / SrcAttn / AttnStack: the one-call eval path runs exactly when ``not training and not grad_enabled``; the
    output carries a graph exactly when grad is enabled and x, coords or the parameters require grad."""
    import warnings

    from hept_amd import ops

    rig = Rig(case, "fp32", dev, precision=precision)
    one_call = []
    for name in ("attn_block_forward", "attn_block_forward_src", "attn_stack_forward", "attn_stack_forward_src"):
        def counted(*a, _fn=getattr(ops, name), _name=name, **kw):
            one_call.append(_name)
            return _fn(*a, **kw)

        monkeypatch.setattr(ops, name, counted)
    mine = {"blk": "attn_block_forward_src" if case.variant == "src" else "attn_block_forward",
            "stack": "attn_stack_forward"}[case.kind]
    for training in (True, False):
        rig.net.train(training)
        for grad in (True, False):
            for req in (set(), {"x"}, {"coords"}, set(rig.param_names), set(rig.all),
                        {nm for nm in rig.param_names if nm.endswith("out_linear.bias")}):
                ins = rig.leaves(req=req)
                del one_call[:]
                for a in rig.ops_:
                    a._warned_eval_grad = False
                with torch.set_grad_enabled(grad), warnings.catch_warnings(record=True) as caught:
                    warnings.simplefilter("always")
                    out = rig.call(*(ins[nm] for nm in rig.input_names))
                what = f"{case.id} {precision} training={training} grad={grad} requires_grad={sorted(req)}"
                assert one_call == ([mine] if not training and not grad else []), (what, one_call)
                # the composed block calls the operator as a trainer would: its documented exception (eval, 16-bit tiles,
                # no gradient into q, k, v or coords) serves the operator's own parameters by the inference path
                excepted = (case.kind == "blk" and not case.fused and precision not in LIGHT and not training and grad
                            and bool(req) and not any(nm in ("x", "coords") + FRONT for nm in req))
                assert len(caught) == (1 if excepted else 0), (what, [str(w.message) for w in caught])
                if excepted:
                    req = req - {"w_rpe.weight", "attn.out_linear.weight", "attn.out_linear.bias"}
                assert out.requires_grad == (grad and bool(req)), what
                if out.requires_grad:
                    out.sum().backward()
                    got = rig.grads(ins)
                    assert {nm for nm, t in got.items() if t is not None} == req, what
    rig.net.train()
