"""MI355X runtime of the CUT3R pointmap network behind the reference's model interface.

Mirrors (same names / argument meaning / outputs) the surface the SLAM trackers use:
    ARCroco3DStereo.from_pretrained(path)          /root/reference/src/dust3r/model.py:305-318
    .normalize(img)                                 :1111-1114
    .encode_image(view) -> (feat, pos, shape)       :1102-1109
    .forward(views, ret_state) / __call__           :894-900, 816-892
and loads the reference state_dict schema (cut3r_slam_amd.config.state_dict_schema).

Execution model: weights are converted once to fp16 [N,K] panels resident in HBM; every operator is a hand-written
gfx950 kernel launched through the C ABI (cut3r_slam_amd.ops); the residual streams stay fp32, GEMM/attention
operands are fp16 with fp32 accumulation (the MI355X has no TF32: fp16-in/fp32-acc MFMA carries the same 10-bit
mantissa the reference's TF32 matmuls do).  The six encoder passes of a window run as ONE batched pass, the DPT
head runs once per window over all views (it does not feed the recurrence), and the dummy zero ray-map encode
(model.py:644-653, multiplied by 0.0) is skipped.
"""
from __future__ import annotations

import contextlib
import gc
import math
import os
import re
from dataclasses import dataclass, field
from typing import Dict, List, NamedTuple, Optional

import torch

from . import ops
from .config import Cut3rConfig, production_config, state_dict_schema

F16, F32 = torch.float16, torch.float32


def _env_flag(name: str, default: bool) -> bool:
    return os.environ.get(name, "1" if default else "0") != "0"


def _env_int(name: str, default: int) -> int:
    return int(os.environ.get(name, str(default)))


@dataclass
class ARCroco3DStereoOutput:          # model.py:50-56 (ModelOutput with ress, views)
    ress: Optional[List[dict]] = None
    views: Optional[List[dict]] = None


class _Lin:
    """fp16 [N,K] weight panel + fp32 bias, N padded up to a multiple of 4 for the vector epilogue."""

    def __init__(self, w: torch.Tensor, b: Optional[torch.Tensor], dev):
        n = w.shape[0]
        self.n = n
        pad = (-n) % 4
        w2 = w.reshape(n, -1).to(F32)
        if pad:
            w2 = torch.cat([w2, torch.zeros(pad, w2.shape[1])], 0)
            if b is not None:
                b = torch.cat([b.to(F32), torch.zeros(pad)], 0)
        self.w = w2.to(device=dev, dtype=F16).contiguous()
        self.b = b.to(device=dev, dtype=F32).contiguous() if b is not None else None
        self.npad = n + pad
        self.k = self.w.shape[1]


class _Stream(NamedTuple):
    """A residual stream of the decoder with its companions of the LayerNorm fold: the GEMM that fills `x` writes them beside it"""
    x: torch.Tensor                          # fp32 [M,C]
    x16: Optional[torch.Tensor] = None       # fp16 copy of x
    st: Optional[torch.Tensor] = None        # slab statistics of its rows, fp32 [C/64, M, 2]


@dataclass
class _Block:
    """One decoder block at work: weights `p`.*, buffers `tag`.*, x fp32 [B*Nx,C] (queries, residual) and y fp32 [B*Ny,C] (keys / values)
    -> out fp32 [B*Nx,C]; B = independent sequences (tracking windows batched through the decoder).  Built by Cut3rModel._block, which
    fills in every field; read by Cut3rModel._dec_layer."""
    p: str
    tag: str
    x: _Stream
    y: _Stream
    out: _Stream
    xpos: Optional[torch.Tensor]             # int64 [B,Nx,2] | None (pose memory: no positions)
    ypos: Optional[torch.Tensor]
    heads: int
    B: int
    pre_ln: bool = False                     # norm1(x) and norm_y(y) are already in `ln16` / `y16` (_dual_norms)
    # derived sizes
    C: int = field(init=False)
    Nx: int = field(init=False)
    Ny: int = field(init=False)
    D: int = field(init=False)               # head width
    # LayerNorms that run inside the projection behind them (decided in _block)
    fold_x: bool = field(init=False, default=False)        # norm1 inside qkv
    fold_y: bool = field(init=False, default=False)        # norm_y inside projk|projv
    fold_o: bool = field(init=False, default=False)        # norm2 inside projq, norm3 inside fc1
    emit: Optional[tuple] = field(init=False, default=None)     # (stats, fp16 copy) of `out` the three residual projections write, when fold_o
    # work buffers `<tag>.<field>`, fp16
    ln16: Optional[torch.Tensor] = field(init=False, default=None)   # [B*Nx,C] norm1 / norm2 / norm3 of the x side
    y16: Optional[torch.Tensor] = field(init=False, default=None)    # [B*Ny,C] norm_y(y)
    qkv: Optional[torch.Tensor] = field(init=False, default=None)    # [B*Nx,3C]
    attn: Optional[torch.Tensor] = field(init=False, default=None)   # [B,Nx,heads,D] self-attention output
    q: Optional[torch.Tensor] = field(init=False, default=None)      # [B,Nx,heads,D] cross-attention queries
    kv: Optional[torch.Tensor] = field(init=False, default=None)     # [B*Ny,2C] cross-attention keys | values
    cattn: Optional[torch.Tensor] = field(init=False, default=None)  # [B,Nx,heads,D] cross-attention output
    mlp_h: Optional[torch.Tensor] = field(init=False, default=None)  # [B*Nx,hidden]

    def __post_init__(self):
        self.C = self.x.x.shape[1]
        self.Nx, self.Ny, self.D = self.x.x.shape[0] // self.B, self.y.x.shape[0] // self.B, self.C // self.heads


class Cut3rModel:
    def __init__(self, cfg: Cut3rConfig, state_dict: Dict[str, torch.Tensor], device="cuda:0", minimal: bool = False):
        """minimal=True computes only what the SLAM trackers consume (pts3d_in_self_view, conf_self, camera_pose:
        hislam2/track_frontend.py:81-100) and skips dpt_cross / dpt_rgb / final_transform."""
        self.cfg = cfg
        self.device = torch.device(device)
        self.minimal = minimal
        schema = state_dict_schema(cfg)
        missing = [k for k in schema if k not in state_dict]
        if missing:
            raise KeyError(f"state_dict is missing {len(missing)} tensors, e.g. {missing[:4]}")
        for k, shp in schema.items():
            if tuple(state_dict[k].shape) != tuple(shp):
                raise ValueError(f"{k}: shape {tuple(state_dict[k].shape)} != schema {tuple(shp)}")
        self._buf: Dict[tuple, torch.Tensor] = {}
        self._graphs: Dict[tuple, tuple] = {}
        # schedule knobs (CUT3R_*): read once here, plain attributes afterwards (tests and tools set them on a constructed model)
        self.use_graphs = _env_flag("CUT3R_GRAPHS", True)            # hipGraph capture / replay per input signature (_graphed)
        self.dual_stream = _env_flag("CUT3R_DUAL_STREAM", True)      # state-side and image-side block of a layer on two capture streams
        self.dual_ln = _env_flag("CUT3R_DUAL_LN", True)              # shared-statistics LayerNorm of the decoder inputs (_dual_norms)
        self.pair_gemm = _env_flag("CUT3R_PAIR_GEMM", False)         # every decoder layer as pair launches: -5 % end to end ("Pair GEMM")
        self.pair_rows = _env_int("CUT3R_PAIR_ROWS", 0)              # pair launches below this many rows: slower at one window too (one-window schedule)
        self.fused_rope = _env_int("CUT3R_FUSED_ROPE", 1)            # RoPE in the q / k projection epilogue: 0 off, 1 heads of 64, 2 also heads of 48 ("RoPE")
        self.rope48_rows = _env_int("CUT3R_ROPE48_ROWS", 0)          # 48-wide heads: fused below this many GEMM rows, 0 never (one-window schedule)
        self.head_overlap = _env_flag("CUT3R_HEAD_OVERLAP", True)    # DPT head of view i on a third stream beside the decoder of view i+1
        self.dpt_fuse = _env_flag("CUT3R_DPT_FUSE", True)            # head.2 + head.4 + activations in one launch
        self.head_chunk = max(1, _env_int("CUT3R_HEAD_CHUNK", 28))   # windows per DPT-head pass of a view ("DPT head chunk")
        # work the result does not need, left out (0: the parent's launches, for A/B runs; same bits): attention over one key and the
        # projections only it reads (pose memory), the view tail and the head inputs written / read in place, q and k RoPE in one launch
        self.one_key = _env_flag("CUT3R_ONE_KEY", True)
        # LayerNorm folded into the GEMMs: 0 off, 1 decoder only, 2 encoder as well ("LayerNorm fold").  The folded panels
        # are built in _prep, so the value can be lowered on a constructed model but not raised
        self.ln_fold = _env_int("CUT3R_LN_FOLD", 1)
        self._head_stream = None
        self._side = None
        self._head_side = None
        # the encoder's static state (the `enc...` buffers, the static input / output of the captured "enc" and "win" graphs) belongs to one
        # stream at a time: (stream, event) of the stream that ran the encoder last, and one reusable event per stream (_encoder_turn)
        self._enc_last = None
        self._enc_events: Dict[int, torch.cuda.Event] = {}
        self._prep(state_dict)

    # ------------------------------------------------------------------ reference-compatible constructors
    @classmethod
    def from_state_dict(cls, cfg, sd, device="cuda:0", **kw):
        return cls(cfg, sd, device, **kw)

    @classmethod
    def from_pretrained(cls, path: str, config: Optional[Cut3rConfig] = None, device="cuda:0", **kw):
        """Load a reference checkpoint (ckpt['model'] = state_dict; ckpt['args'].model = constructor string,
        model.py:72-92).  Only weights_only loading is used; the constructor string is parsed, never eval'd."""
        import argparse
        if not os.path.isfile(path):
            raise FileNotFoundError(f"{path}: no checkpoint (this runtime never fetches from a hub)")
        with torch.serialization.safe_globals([argparse.Namespace]):
            ckpt = torch.load(path, map_location="cpu", weights_only=True)
        sd = ckpt["model"] if "model" in ckpt else ckpt
        sd = {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}
        if not any(k.startswith("dec_blocks_state") for k in sd):       # model.py:390-393
            for k in list(sd):
                if k.startswith("dec_blocks"):
                    sd[k.replace("dec_blocks", "dec_blocks_state")] = sd[k]
        if config is None:
            config = production_config()
            args = getattr(ckpt.get("args", None), "model", "") if isinstance(ckpt, dict) else ""
            config = _config_from_ctor_string(args, config)
        return cls(config, sd, device, **kw)

    def to(self, device):
        return self

    def eval(self):
        return self

    # ------------------------------------------------------------------ weight preparation
    def _prep(self, sd):
        cfg, dev = self.cfg, self.device
        f32 = lambda k: sd[k].to(device=dev, dtype=F32).contiguous()
        self.w: Dict[str, object] = {}

        def lin(name, key=None):
            key = key or name
            self.w[name] = _Lin(sd[key + ".weight"], sd.get(key + ".bias"), dev)

        def ln(name):
            self.w[name] = (f32(name + ".weight"), f32(name + ".bias"))

        def fold(name, w, b, norm):
            """LayerNorm `norm` folded into the Linear (w, b) that consumes it: y = LN(x) W^T + b = rstd (x (gamma.W)^T - mu c) + d with the
            panel fp16(gamma . W), c_n = the row sums of THAT panel (so the constant part cancels exactly) and d = W beta + b"""
            if not self.ln_fold or w.shape[1] % 64 or w.shape[0] % 4 or w.shape[1] > ops.LN_FOLD_MAX_K:
                return              # wider rows than the folded epilogue normalises keep their LayerNorm launch
            gam, bet = sd[norm + ".weight"].double(), sd[norm + ".bias"].double()
            wd = w.double()
            L = _Lin((wd * gam[None, :]).float(), None, dev)
            L.b = (wd @ bet + b.double()).to(device=dev, dtype=F32).contiguous()
            L.c = L.w.double().sum(1).to(F32).contiguous()
            self.w[name + "@ln"] = L

        def enc_block(p):
            ln(p + ".norm1"); lin(p + ".attn.qkv"); lin(p + ".attn.proj"); ln(p + ".norm2")
            lin(p + ".mlp.fc1"); lin(p + ".mlp.fc2")
            if self.ln_fold >= 2:
                fold(p + ".attn.qkv", sd[p + ".attn.qkv.weight"], sd[p + ".attn.qkv.bias"], p + ".norm1")
                fold(p + ".mlp.fc1", sd[p + ".mlp.fc1.weight"], sd[p + ".mlp.fc1.bias"], p + ".norm2")

        def dec_block(p, folded=True):
            ln(p + ".norm1"); lin(p + ".attn.qkv"); lin(p + ".attn.proj")
            ln(p + ".norm2"); ln(p + ".norm3"); ln(p + ".norm_y")
            lin(p + ".cross_attn.projq"); lin(p + ".cross_attn.proj")
            wkv = torch.cat([sd[p + ".cross_attn.projk.weight"], sd[p + ".cross_attn.projv.weight"]], 0)
            bkv = torch.cat([sd[p + ".cross_attn.projk.bias"], sd[p + ".cross_attn.projv.bias"]], 0)
            self.w[p + ".cross_attn.projkv"] = _Lin(wkv, bkv, dev)
            lin(p + ".mlp.fc1"); lin(p + ".mlp.fc2")
            if folded:
                fold(p + ".attn.qkv", sd[p + ".attn.qkv.weight"], sd[p + ".attn.qkv.bias"], p + ".norm1")
                fold(p + ".cross_attn.projq", sd[p + ".cross_attn.projq.weight"], sd[p + ".cross_attn.projq.bias"], p + ".norm2")
                fold(p + ".cross_attn.projkv", wkv, bkv, p + ".norm_y")
                fold(p + ".mlp.fc1", sd[p + ".mlp.fc1.weight"], sd[p + ".mlp.fc1.bias"], p + ".norm3")

        self.w["patch_embed"] = _Lin(sd["patch_embed.proj.weight"], sd["patch_embed.proj.bias"], dev)
        for i in range(cfg.enc_depth):
            enc_block(f"enc_blocks.{i}")
        ln("enc_norm")
        lin("decoder_embed"); lin("decoder_embed_state")
        for i in range(cfg.dec_depth):
            dec_block(f"dec_blocks.{i}"); dec_block(f"dec_blocks_state.{i}")
        ln("dec_norm"); ln("dec_norm_state")
        lin("pose_retriever.proj_q")
        for i in range(2):
            dec_block(f"pose_retriever.write_blocks.{i}", False); dec_block(f"pose_retriever.read_blocks.{i}", False)
        self.pose_token = f32("pose_token").reshape(1, -1)
        self.masked_token = f32("pose_retriever.masked_token").reshape(1, -1)
        self.mem0 = f32("pose_retriever.mem").reshape(cfg.local_mem_size, -1)
        self.register_tokens16 = sd["register_tokens.weight"].to(device=dev, dtype=F16).contiguous()
        w = cfg.state_width
        i = torch.arange(cfg.state_size)
        self.state_pos = torch.stack([i // w, i % w], -1)[None].to(dev).contiguous()       # int64 [1,S,2]
        for hd in {cfg.enc_embed_dim // cfg.enc_num_heads, cfg.dec_embed_dim // cfg.dec_num_heads, cfg.dec_embed_dim // cfg.state_dec_num_heads}:
            if hd % 16 == 0:
                ops.rope_table(dev, cfg.rope_freq, 1.0, hd)        # cos|sin tables of the RoPE launches: filled before any graph capture
        h = "downstream_head"
        lin(h + ".pose_head.mlp.fc1"); lin(h + ".pose_head.mlp.fc2")
        if cfg.head_type == "dpt":
            self._prep_dpt(sd, h + ".dpt_self", 4)
            if not self.minimal:
                self._prep_dpt(sd, h + ".dpt_cross", 4)
                if cfg.rgb_head:
                    self._prep_dpt(sd, h + ".dpt_rgb", 3)
        else:
            lin(h + ".proj.fc1"); lin(h + ".proj.fc2")
            if not self.minimal:
                lin(h + ".cross_proj.fc1"); lin(h + ".cross_proj.fc2")
                if cfg.rgb_head:
                    lin(h + ".rgb_proj.fc1"); lin(h + ".rgb_proj.fc2")
        if not self.minimal:
            for i in range(2):
                p = f"{h}.final_transform.{i}"
                for n in ("norm1", "norm2"):
                    ln(f"{p}.{n}.norm"); lin(f"{p}.{n}.mlp.1")
                lin(p + ".attn.qkv"); lin(p + ".attn.proj"); lin(p + ".mlp.fc1"); lin(p + ".mlp.fc2")

    def _prep_dpt(self, sd, p, nch):
        dev = self.device

        def c3(name):
            w = sd[name + ".weight"]                                  # [Cout,Cin,3,3] -> [Cout,(ky,kx,ci)]
            self.w[name] = _Lin(w.permute(0, 2, 3, 1).reshape(w.shape[0], -1), sd.get(name + ".bias"), dev)

        def c1(name):
            w = sd[name + ".weight"]
            self.w[name] = _Lin(w.reshape(w.shape[0], -1), sd.get(name + ".bias"), dev)

        def ct(name):
            w = sd[name + ".weight"]                                  # [Cin,Cout,k,k] -> [(i,j,co), ci]
            k = w.shape[2]
            l = _Lin(w.permute(2, 3, 1, 0).reshape(k * k * w.shape[1], w.shape[0]), None, dev)
            l.b = sd[name + ".bias"].to(device=dev, dtype=F32).contiguous()
            l.s = k
            self.w[name] = l

        a = p + ".act_postprocess"
        c1(a + ".0.0"); ct(a + ".0.1"); c1(a + ".1.0"); ct(a + ".1.1"); c1(a + ".2.0"); c1(a + ".3.0"); c3(a + ".3.1")
        for i in range(4):
            c3(f"{p}.scratch.layer_rn.{i}")
        for r in (1, 2, 3, 4):
            q = f"{p}.scratch.refinenet{r}"
            c1(q + ".out_conv")
            for u in ("resConfUnit1", "resConfUnit2"):
                c3(f"{q}.{u}.conv1"); c3(f"{q}.{u}.conv2")
        c3(p + ".head.0"); c3(p + ".head.2")
        self.w[p + ".head.4.w"] = sd[p + ".head.4.weight"].reshape(nch, -1).to(device=dev, dtype=F32).contiguous()
        self.w[p + ".head.4.b"] = sd[p + ".head.4.bias"].to(device=dev, dtype=F32).contiguous()

    # ------------------------------------------------------------------ buffers
    def buf(self, name, shape, dtype):
        key = (name, tuple(shape), dtype)
        t = self._buf.get(key)
        if t is None:
            t = torch.empty(shape, dtype=dtype, device=self.device)
            self._buf[key] = t
        return t

    # ------------------------------------------------------------------ primitives
    def _panel(self, name, rope=None, ln=None):
        """the weight panel of Linear `name` with the rope / ln arguments as ops.linear and ops.linear_pair take them:
        rope = (positions [B,N,2], cols, head width) -> + the RoPE base; ln = slab statistics -> the folded panel `name@ln`, its column sums, eps"""
        L = self.w[name + "@ln"] if ln is not None else self.w[name]
        if rope is not None:
            rope = (rope[0], rope[1], self.cfg.rope_freq, rope[2])
        if ln is not None:
            ln = (ln, L.c, self.cfg.ln_eps)
        return L, rope, ln

    def _linear(self, x16, name, out, act=0, res1=None, res2=None, skinny=False, rope=None, ln=None, emit=None, cols=None):
        """skinny: the operand has ONE row per independent sequence (pose token of a tracking window): weight-streaming
        kernel whose per-row result does not depend on how many windows are batched.
        rope = (positions [B,N,2], cols, head width): RoPE of the first `cols` output columns fused into the GEMM epilogue.
        ln = slab statistics of the rows of `x16` (then x16 is the fp16 copy of the UN-normalised residual stream and the LayerNorm in front
        of this Linear runs inside its epilogue through the folded panel `name@ln`); emit = (stats, x16) this GEMM writes for the next one.
        cols = (lo, hi): only the output columns lo..hi (contiguous weight rows and bias) -- skinny only: that kernel computes every output
        column on its own, in an order that depends on K alone, so the columns keep their bits."""
        L, rope, ln = self._panel(name, rope, ln)
        w, b = L.w, L.b
        if cols is not None:
            assert skinny and rope is None and ln is None and emit is None, "a column range: the skinny kernel only"
            w, b = w[cols[0]:cols[1]], (b[cols[0]:cols[1]] if b is not None else None)
        return ops.linear(x16, w, out, b, act, res1, res2, tile=16 if skinny else 0, rope=rope, ln=ln, emit=emit)

    def _project(self, probs, act=0):
        """one projection step of a decoder layer, probs = the keyword arguments of `_linear` per block: one block -> ops.linear; the state-side
        and the image-side block -> both problems in ONE grid (ops.linear_pair; same rows, bit for bit)"""
        if not probs:
            return None
        if len(probs) == 1:
            return self._linear(act=act, **probs[0])

        def prob(x16, name, out, res1=None, skinny=False, rope=None, ln=None, emit=None):
            assert not skinny, "the pair kernels have no one-row-per-sequence form"
            L, rope, ln = self._panel(name, rope, ln)
            return (x16, L.w, out, L.b, res1, dict(rope=rope, ln=ln, emit=emit))
        ops.linear_pair(prob(**probs[0]), prob(**probs[1]), act)

    def _folded(self, name):
        return self.ln_fold and (name + "@ln") in self.w

    def _xs(self, tag, x):
        """the fp16 copy + slab statistics that belong to the fp32 residual buffer `x` ([M,C], C % 64 == 0): (x16, stats [C/64, M, 2])"""
        M, Cc = x.shape
        return self.buf(tag + ".x16", (M, Cc), F16), self.buf(tag + ".xst", (Cc // 64, M, 2), F32)

    def _fuse_rope(self, pos, D, rows):
        """the GEMM-fused RoPE covers head dimension 64 with one position row per GEMM row; 48-wide heads (the state side of the decoder)
        need the 128 x 192 tile, which loses to the 256 x 256 kernel + a RoPE launch on large batches (round 3: -3 % end to end at 28
        windows) but shortens the launch chain of the one-window schedule, where every launch is latency: fused up to `rope48_rows` rows"""
        dims = (64, 48) if (self.fused_rope == 2 or (self.fused_rope and rows <= self.rope48_rows)) else (64,)
        return self.fused_rope and pos is not None and D in dims and pos.is_contiguous() and pos.numel() == 2 * rows

    def _ln(self, x, name, out16=None, out32=None, mod=None):
        g, b = self.w[name]
        ops.layernorm(x, g, b, self.cfg.ln_eps, out16, out32, mod[0] if mod else None, mod[1] if mod else None)

    def _rope(self, t, pos):
        ops.rope_2d_pair(t, pos, None, None, self.cfg.rope_freq, 1.0)

    def _self_attn(self, tag, x_ln16, B, N, heads, pos, p, out, res, ln=None, emit=None):
        """x_ln16 fp16 [B*N,C] -> out(fp32) = res + proj(attn(qkv(x))).  ln: x_ln16 is the UN-normalised fp16 copy and `ln` its slab
        statistics (norm1 folded into qkv); emit: the projection also writes (stats, fp16 copy) of `out`."""
        Cc = x_ln16.shape[1]
        D = Cc // heads
        sk = N == 1
        qkv = self.buf(tag + ".qkv", (B * N, 3 * Cc), F16)
        fuse = (not sk) and self._fuse_rope(pos, D, B * N)
        self._linear(x_ln16, p + ".qkv", qkv, skinny=sk, rope=(pos, 2 * Cc, D) if fuse else None, ln=ln)
        v5 = qkv.view(B, N, 3, heads, D)
        q, k, v = v5[:, :, 0], v5[:, :, 1], v5[:, :, 2]
        if pos is not None and not fuse:
            ops.rope_2d_pair(q, pos, k, pos, self.cfg.rope_freq, 1.0)
        a = self.buf(tag + ".attn", (B, N, heads, D), F16)
        ops.attention(q, k, v, a, D ** -0.5)
        self._linear(a.view(B * N, Cc), p + ".proj", out, res1=res, skinny=sk, emit=emit)

    def _mlp(self, tag, x_ln16, p, out, res, ln=None, emit=None):
        M = x_ln16.shape[0]
        hdim = self.w[p + ".fc1"].npad
        h = self.buf(tag + ".mlp_h", (M, hdim), F16)
        self._linear(x_ln16, p + ".fc1", h, act=1, ln=ln)
        self._linear(h, p + ".fc2", out, res1=res, emit=emit)

    # ------------------------------------------------------------------ encoder
    @contextlib.contextmanager
    def _encoder_turn(self):
        """One encoder pass at a time, whichever stream issues it: the pass that ran last left an event, and a pass on ANOTHER stream makes
        its stream wait for that event before it touches the encoder's static state (eager: the `enc...` buffers; graphs: static input and
        output of the "enc" / "win" replays, through the caller's copy of the output).  Stream-side waits only, no host synchronisation;
        with one stream in use nothing is waited for, and nothing at all happens inside a capture (the guard sits around the replay).
        Decoder passes are not ordered against it: a look-ahead encoder pass still runs beside the windows of the main stream
        (`decode_window` / `decode_windows`, the trackers' path).  Two exceptions, both stated here: the graphed `forward_window` of IMAGES
        is one replay of encoder + decoder + heads that cannot be split, so it takes its turn as a whole; and in graph mode `encode_image`
        returns `pos` as the static output of the replay, read outside the turn -- every replay of a shape writes the same positions."""
        if torch.cuda.is_current_stream_capturing():
            yield
            return
        cur = torch.cuda.current_stream()
        last = self._enc_last
        if last is not None and last[0] != cur:
            cur.wait_event(last[1])
        try:
            yield
        finally:
            ev = self._enc_events.get(cur.cuda_stream)
            if ev is None:
                ev = self._enc_events[cur.cuda_stream] = torch.cuda.Event()
            ev.record(cur)
            self._enc_last = (cur, ev)

    def _encode(self, img: torch.Tensor):
        """img [B,3,H,W] (fp32 normalised, or uint8 -> normalisation fused).  Returns fp32 feat [B,N,E], fp16 copy."""
        with self._encoder_turn():
            return self._encode_pass(img)

    def _encode_pass(self, img: torch.Tensor):
        cfg = self.cfg
        B, _, H, W = img.shape
        P, E = cfg.patch_size, cfg.enc_embed_dim
        nh, nw = H // P, W // P
        N = nh * nw
        M = B * N
        tag = f"enc{B}x{N}"
        patches = self.buf(tag + ".patches", (M, 3 * P * P), F16)
        ops.im2col_patch(img.contiguous(), P, patches)
        x = self.buf(tag + ".x", (M, E), F32)
        self._linear(patches, "patch_embed", x)
        y, xx = torch.meshgrid(torch.arange(nh, device=self.device), torch.arange(nw, device=self.device), indexing="ij")
        pos = torch.stack([y.reshape(-1), xx.reshape(-1)], -1)[None].expand(B, -1, -1).contiguous()
        ln16 = self.buf(tag + ".ln16", (M, E), F16)
        fold = self.ln_fold >= 2 and self._folded("enc_blocks.0.attn.qkv") and E % 64 == 0
        x16, xst = self._xs(tag, x) if fold else (None, None)
        em = (xst, x16) if fold else None
        for i in range(cfg.enc_depth):
            p = f"enc_blocks.{i}"
            if fold and i > 0:           # norm1 runs inside the qkv epilogue, on the copy + statistics the previous block's fc2 wrote
                self._self_attn(tag, x16, B, N, cfg.enc_num_heads, pos, p + ".attn", x, x, ln=xst, emit=em)
            else:
                self._ln(x, p + ".norm1", out16=ln16)
                self._self_attn(tag, ln16, B, N, cfg.enc_num_heads, pos, p + ".attn", x, x, emit=em)
            if fold:                     # norm2 inside the fc1 epilogue
                self._mlp(tag, x16, p + ".mlp", x, x, ln=xst, emit=em if i + 1 < cfg.enc_depth else None)
            else:
                self._ln(x, p + ".norm2", out16=ln16)
                self._mlp(tag, ln16, p + ".mlp", x, x)
        feat = torch.empty((B, N, E), dtype=F32, device=self.device)
        feat16 = torch.empty((B, N, E), dtype=F16, device=self.device)
        self._ln(x, "enc_norm", out16=feat16.view(M, E), out32=feat.view(M, E))
        return feat, feat16, pos

    # ------------------------------------------------------------------ hipGraph capture
    def _graphed(self, kind, fn, inp):
        """Capture `fn(static_input)` once per input signature into a hipGraph and replay it: a window is ~4000 kernel
        launches, which the Python/ctypes host path cannot issue as fast as the GPU retires them.  Inputs are copied
        into a static buffer; outputs are static tensors that the caller must consume before the next replay."""
        key = (kind, tuple(inp.shape), inp.dtype)      # `kind` may itself be a tuple (e.g. image size)
        ent = self._graphs.get(key)
        if ent is None:
            static_in = inp.clone()
            cur = torch.cuda.current_stream()
            side = torch.cuda.Stream()
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                for _ in range(2):          # warm-up: creates every persistent workspace outside the capture
                    fn(static_in)
            cur.wait_stream(side)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            # no garbage collection while the stream is capturing: a collected tensor / graph of a dead model would be
            # released (hipFree, hipGraphExecDestroy) in the middle of the capture
            gc_was_on = gc.isenabled()
            gc.collect()
            gc.disable()
            try:
                with torch.cuda.graph(graph):
                    out = fn(static_in)
            finally:
                if gc_was_on:
                    gc.enable()
            ent = (graph, static_in, out)
            self._graphs[key] = ent
        graph, static_in, out = ent
        static_in.copy_(inp, non_blocking=True)
        graph.replay()
        return out

    def normalize(self, img_tensor):
        return (img_tensor / 255.0 - 0.5) / 0.5

    def encode_image(self, view):
        img = view["img"]
        if not img.is_cuda:
            img = img.to(self.device)
        B = img.shape[0]
        im_shape = view.get("true_shape", torch.tensor(img.shape[-2:])[None].repeat(B, 1))
        img = img.to(F32) if img.dtype != torch.uint8 else img
        if self.use_graphs:
            with self._encoder_turn():
                feat, _, pos = self._graphed("enc", self._encode, img.contiguous())
                feat = feat.clone()        # callers keep encoder features (keyframe store)
        else:
            feat, _, pos = self._encode(img)
        return feat, pos, im_shape

    # ------------------------------------------------------------------ decoder layer
    def _block(self, p, tag, x, y, out, xpos, ypos, heads, B=1, fresh=False, pre_ln=False):
        """One decoder block as `_dec_layer` takes it, with its work buffers `<tag>.*` and -- here and nowhere else -- which of its LayerNorms
        run folded into the projection behind them: the fold is on, the panel `name@ln` exists, the stream carries valid companions and the
        operand has more than one row per sequence (the skinny kernel has no folded form).  fresh: the companions of x and y were written
        by the GEMMs that filled them (those of `out` are written by this block itself); pre_ln: see _Block."""
        s = _Block(p, tag, x, y, out, xpos, ypos, heads, B, pre_ln)
        C, Nx, Ny, D = s.C, s.Nx, s.Ny, s.D
        can = lambda t, n, name: bool(t.x16 is not None and n > 1 and self._folded(p + name))
        s.fold_x = fresh and can(x, Nx, ".attn.qkv")                   # norm1 inside qkv
        s.fold_y = fresh and can(y, Ny, ".cross_attn.projkv")          # norm_y inside projk|projv
        s.fold_o = can(out, Nx, ".mlp.fc1")                            # norm2 inside projq, norm3 inside fc1
        s.emit = (out.st, out.x16) if s.fold_o else None               # (stats, fp16 copy) the three residual projections write
        s.ln16 = self.buf(tag + ".ln16", (B * Nx, C), F16)
        s.y16 = self.buf(tag + ".y16", (B * Ny, C), F16)
        s.qkv = self.buf(tag + ".qkv", (B * Nx, 3 * C), F16)
        s.attn = self.buf(tag + ".attn", (B, Nx, heads, D), F16)
        s.q = self.buf(tag + ".q", (B, Nx, heads, D), F16)
        s.kv = self.buf(tag + ".kv", (B * Ny, 2 * C), F16)
        s.cattn = self.buf(tag + ".cattn", (B, Nx, heads, D), F16)
        s.mlp_h = self.buf(tag + ".mlp_h", (B * Nx, self.w[p + ".mlp.fc1"].npad), F16)
        return s

    def _pair_carries(self, rows):
        """What the pair launches may carry: below `pair_rows` rows (the one-window schedule) they run on the 64 x 64 pair kernels, which take
        the LayerNorm fold and the fused RoPE of 64-wide heads; a forced pair form (`pair_gemm`) on a larger batch runs the plain 128 / 256
        pair kernels -- no fold, no fused RoPE, LayerNorm and RoPE launches instead.  rows = the largest operand of the layer."""
        return rows <= self.pair_rows

    def _dec_layer(self, blocks, fork=False):
        """The decoder block (dust3r/blocks.py:292-297: x += attn(norm1 x); x += cross_attn(norm2 x, norm_y y); x += mlp(norm3 x)) for ONE block,
        or for the state-side and the image-side block of a layer together (model.py:669-692: both read the previous layer's pair, so they
        are independent).  Together, each of the seven projections is one pair launch (`_project`) while LayerNorm, RoPE and attention stay
        per block (different token counts and head widths) -- under graph capture with `fork` on the two capture streams.  Same kernels, same
        row arithmetic: the results do not depend on the form."""
        pair = len(blocks) == 2
        assert not pair or all(s.Nx > 1 and s.Ny > 1 for s in blocks), "pair launches need more than one row per sequence"
        carry = pair and self._pair_carries(max(s.B * max(s.Nx, s.Ny) for s in blocks))
        assert not pair or carry or not any(s.fold_x or s.fold_y or s.fold_o for s in blocks), "the plain pair kernels take no LayerNorm fold"
        # RoPE of q / k in the projection's epilogue (else a launch behind it): `_fuse_rope`; the pair kernels: heads of 64
        fuse = lambda s, pos, n: bool(n > 1 and self._fuse_rope(pos, s.D, s.B * n) and (not pair or (carry and s.D == 64)))
        fuse_x, fuse_y = (lambda s: fuse(s, s.xpos, s.Nx)), (lambda s: fuse(s, s.ypos, s.Ny))

        def each(fn, need=lambda s: True):
            """a step that runs per block: fn(block) for those that need it"""
            todo = [s for s in blocks if need(s)]
            if fork and len(todo) == 2:
                cur = torch.cuda.current_stream()
                self._side.wait_stream(cur)
                with torch.cuda.stream(self._side):
                    fn(todo[0])
                fn(todo[1])
                cur.wait_stream(self._side)
            else:
                for s in todo:
                    fn(s)

        rows = lambda t: t.view(-1, t.shape[-2] * t.shape[-1])        # [B,N,heads,D] -> [B*N,C]
        skx, sky = (lambda s: s.Nx == 1), (lambda s: s.Ny == 1)
        # one key: its softmax is 1 and the attention output is the value row (ops.attention_one_key), so q and k are never read.  Self
        # attention of ONE token (Nx == 1, the pose-memory read blocks): only the V columns of qkv are projected, straight into `attn`
        # (every skx projection is the skinny kernel at any B -- ops.linear chunks it -- which `_linear(cols=)` needs).  Cross attention to
        # ONE token (Ny == 1, the write blocks): no norm2, no projq, no q RoPE
        one_x, one_y = (lambda s: self.one_key and s.Nx == 1), (lambda s: self.one_key and s.Ny == 1)
        # ---- self attention
        each(lambda s: self._ln(s.x.x, s.p + ".norm1", out16=s.ln16), lambda s: not (s.fold_x or s.pre_ln))
        self._project([dict(x16=s.x.x16 if s.fold_x else s.ln16, name=s.p + ".attn.qkv", out=s.qkv, skinny=skx(s),
                            rope=(s.xpos, 2 * s.C, s.D) if fuse_x(s) else None, ln=s.x.st if s.fold_x else None)
                       if not one_x(s) else
                       dict(x16=s.ln16, name=s.p + ".attn.qkv", out=rows(s.attn), skinny=True, cols=(2 * s.C, 3 * s.C)) for s in blocks])

        def self_attn(s):
            v5 = s.qkv.view(s.B, s.Nx, 3, s.heads, s.D)
            q, k, v = v5[:, :, 0], v5[:, :, 1], v5[:, :, 2]
            if s.xpos is not None and not fuse_x(s):
                ops.rope_2d_pair(q, s.xpos, k, s.xpos, self.cfg.rope_freq, 1.0)
            ops.attention(q, k, v, s.attn, s.D ** -0.5)
        each(self_attn, lambda s: not one_x(s))
        self._project([dict(x16=rows(s.attn), name=s.p + ".attn.proj", out=s.out.x, res1=s.x.x, skinny=skx(s), emit=s.emit) for s in blocks])
        # ---- cross attention: queries from x, keys / values from y
        each(lambda s: self._ln(s.out.x, s.p + ".norm2", out16=s.ln16), lambda s: not (s.fold_o or one_y(s)))
        self._project([dict(x16=s.out.x16 if s.fold_o else s.ln16, name=s.p + ".cross_attn.projq", out=rows(s.q), skinny=skx(s),
                            rope=(s.xpos, s.C, s.D) if fuse_x(s) else None, ln=s.out.st if s.fold_o else None) for s in blocks if not one_y(s)])
        rope_q = lambda s: s.xpos is not None and not fuse_x(s) and not one_y(s)
        rope_k = lambda s: s.ypos is not None and not fuse_y(s) and not one_y(s)
        # q and k both rotated by a launch (the 48-wide heads): ONE launch behind projk|projv covers both token ranges
        rope_qk = lambda s: self.one_key and rope_q(s) and rope_k(s)
        norm_y = lambda s: not (s.fold_y or s.pre_ln)

        def q_rope_and_norm_y(s):
            if rope_q(s) and not rope_qk(s):
                self._rope(s.q, s.xpos)
            if norm_y(s):
                self._ln(s.y.x, s.p + ".norm_y", out16=s.y16)
        each(q_rope_and_norm_y, lambda s: (rope_q(s) and not rope_qk(s)) or norm_y(s))
        self._project([dict(x16=s.y.x16 if s.fold_y else s.y16, name=s.p + ".cross_attn.projkv", out=s.kv, skinny=sky(s),
                            rope=(s.ypos, s.C, s.D) if fuse_y(s) else None, ln=s.y.st if s.fold_y else None) for s in blocks])

        def cross_attn(s):
            kv4 = s.kv.view(s.B, s.Ny, 2, s.heads, s.D)
            k, v = kv4[:, :, 0], kv4[:, :, 1]
            if one_y(s):
                return ops.attention_one_key(v, s.cattn)
            if rope_qk(s):
                ops.rope_2d_pair(s.q, s.xpos, k, s.ypos, self.cfg.rope_freq, 1.0)
            elif s.ypos is not None and not fuse_y(s):
                self._rope(k, s.ypos)
            ops.attention(s.q, k, v, s.cattn, s.D ** -0.5)
        each(cross_attn)
        self._project([dict(x16=rows(s.cattn), name=s.p + ".cross_attn.proj", out=s.out.x, res1=s.out.x, skinny=skx(s), emit=s.emit) for s in blocks])
        # ---- MLP
        each(lambda s: self._ln(s.out.x, s.p + ".norm3", out16=s.ln16), lambda s: not s.fold_o)
        self._project([dict(x16=s.out.x16 if s.fold_o else s.ln16, name=s.p + ".mlp.fc1", out=s.mlp_h, skinny=skx(s),
                            ln=s.out.st if s.fold_o else None) for s in blocks], act=1)
        self._project([dict(x16=s.mlp_h, name=s.p + ".mlp.fc2", out=s.out.x, res1=s.out.x, skinny=skx(s), emit=s.emit) for s in blocks])

    def _dual_norms(self, l, a, s_a):
        """The four input norms of decoder layer l in two launches: the image tokens `a` feed norm1 of the image block and
        norm_y of the state block, the state tokens `s_a` feed norm1 of the state block and norm_y of the image block; each
        tensor is read once and its row statistics are shared (identical outputs to four separate LayerNorms)."""
        pi, ps = f"dec_blocks.{l}", f"dec_blocks_state.{l}"
        Ci = a.shape[1]
        ops.layernorm_dual(a, *self.w[pi + ".norm1"], self.buf("deci.ln16", (a.shape[0], Ci), F16),
                           *self.w[ps + ".norm_y"], self.buf("decs.y16", (a.shape[0], Ci), F16), self.cfg.ln_eps)
        ops.layernorm_dual(s_a, *self.w[ps + ".norm1"], self.buf("decs.ln16", (s_a.shape[0], Ci), F16),
                           *self.w[pi + ".norm_y"], self.buf("deci.y16", (s_a.shape[0], Ci), F16), self.cfg.ln_eps)

    # ------------------------------------------------------------------ pose memory
    def _mem_inquire(self, gfeat16, mem, B=1):
        """gfeat16 [B,E] fp16, mem [B*size, 2D] -> pose feature [B, D]  (model.py:217-222)"""
        cfg = self.cfg
        D = cfg.dec_embed_dim
        x = self.buf("memr.x", (B, 2 * D), F32)
        self._linear(gfeat16, "pose_retriever.proj_q", x[:, :D], skinny=True)
        x[:, D:] = self.masked_token
        a, b, m = _Stream(x), _Stream(self.buf("memr.x2", (B, 2 * D), F32)), _Stream(mem)
        for i in range(2):
            self._dec_layer([self._block(f"pose_retriever.read_blocks.{i}", "memr", a, m, b, None, None, cfg.dec_num_heads, B)])
            a, b = b, a
        return a.x[:, D:]

    def _mem_update(self, mem, gfeat16, pose_out, out, B=1):
        """mem [B*size, 2D], pose_out [B, D] -> out (new memory)  (model.py:204-215)"""
        cfg = self.cfg
        D = cfg.dec_embed_dim
        f = self.buf("memw.f", (B, 2 * D), F32)
        self._linear(gfeat16, "pose_retriever.proj_q", f[:, :D], skinny=True)
        f[:, D:] = pose_out
        m, f, tmp, o = _Stream(mem), _Stream(f), _Stream(self.buf("memw.tmp", tuple(mem.shape), F32)), _Stream(out)
        self._dec_layer([self._block("pose_retriever.write_blocks.0", "memw", m, f, tmp, None, None, cfg.dec_num_heads, B)])
        self._dec_layer([self._block("pose_retriever.write_blocks.1", "memw", tmp, f, o, None, None, cfg.dec_num_heads, B)])
        return out

    # ------------------------------------------------------------------ heads
    def _conv3(self, x, name, stride=1, relu_in=False, act=0, res1=None, res2=None, tag=None):
        L = self.w[name]
        B, H, W, _ = x.shape
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        out = self.buf(tag or name, (B, Ho, Wo, L.npad), F16)
        return ops.conv3x3_nhwc(x, L.w, out, L.b, stride, relu_in, act, res1, res2)

    def _conv1(self, x, name, tag=None):
        L = self.w[name]
        B, H, W, Cc = x.shape
        out = self.buf(tag or name, (B, H, W, L.npad), F16)
        if x.is_contiguous():
            ops.linear(x.view(-1, Cc), L.w, out.view(-1, L.npad), L.b)
        else:       # one view of several windows, read where it lies (batch stride = one window): a problem per batch element, same bits
            ops.linear_batched(x.view(B, H * W, Cc), L.w.unsqueeze(0).expand(B, -1, -1), out.view(B, H * W, L.npad),
                               None if L.b is None else L.b.unsqueeze(0).expand(B, -1))
        return out

    def _convT(self, x, name):
        L = self.w[name]
        B, H, W, Cc = x.shape
        cout = L.npad // (L.s * L.s)
        out = self.buf(name, (B, H * L.s, W * L.s, cout), F16)
        return ops.conv_transpose_nhwc(x, L.w, out, L.b, L.s)

    def _up2(self, x, tag):
        B, H, W, Cc = x.shape
        return ops.upsample2x(x, self.buf(tag, (B, 2 * H, 2 * W, Cc), F16))

    def _rcu(self, x, p, res2=None):
        t = self._conv3(x, p + ".conv1", relu_in=True, act=2)
        return self._conv3(t, p + ".conv2", res1=x, res2=res2)

    def _fusion(self, p, x0, x1=None):
        out = x0 if x1 is None else self._rcu(x1, p + ".resConfUnit1", res2=x0)
        out = self._rcu(out, p + ".resConfUnit2")
        out = self._up2(out, p + ".up")
        return self._conv1(out, p + ".out_conv")

    def _dpt(self, p, toks16: List[torch.Tensor], B, nh, nw, last=True):
        """toks16: 4 fp16 tensors [B*nh*nw, C_i] (NHWC token maps), or [B, nh*nw, C_i] views with a batch stride.  Returns fp16 [B*H*W, last_dim] features (last=False: the
        input of head.2, for a caller that runs head.2 together with the output stage)."""
        a = p + ".act_postprocess"
        t = [x.view(B, nh, nw, -1) for x in toks16]
        l0 = self._convT(self._conv1(t[0], a + ".0.0"), a + ".0.1")
        l1 = self._convT(self._conv1(t[1], a + ".1.0"), a + ".1.1")
        l2 = self._conv1(t[2], a + ".2.0")
        l3 = self._conv3(self._conv1(t[3], a + ".3.0"), a + ".3.1", stride=2)
        L = [self._conv3(l, f"{p}.scratch.layer_rn.{i}") for i, l in enumerate((l0, l1, l2, l3))]
        p4 = self._fusion(p + ".scratch.refinenet4", L[3])
        if p4.shape[1] != L[2].shape[1] or p4.shape[2] != L[2].shape[2]:
            p4 = p4[:, : L[2].shape[1], : L[2].shape[2]].contiguous()          # dpt_head.py:63-65 crop
        p3 = self._fusion(p + ".scratch.refinenet3", p4, L[2])
        p2 = self._fusion(p + ".scratch.refinenet2", p3, L[1])
        p1 = self._fusion(p + ".scratch.refinenet1", p2, L[0])
        o = self._conv3(p1, p + ".head.0")
        o = self._up2(o, p + ".head.up")
        if last:
            o = self._conv3(o, p + ".head.2", act=2)
        return o

    def _dpt_fused(self, p):
        """head.2 + head.4 + activations in one launch (CUT3R_DPT_FUSE=0: the two launches, for A/B runs)"""
        L = self.w[p + ".head.2"]
        return self.dpt_fuse and L.b is not None and ops.conv3x3_dpt_final_ok(L.w.shape[1] // 9, L.npad, self.w[p + ".head.4.w"])

    def _dpt_pts(self, p, toks16, B, nh, nw, H, W, key_pts, key_conf, res, out=None):
        """out = (pts [B,H,W,3], conf [B,H,W]): contiguous, or -- on the fused path only -- contiguous views a constant stride apart"""
        fused = self._dpt_fused(p)
        o = self._dpt(p, toks16, B, nh, nw, last=not fused)
        if out is None:
            pts = torch.empty((B, H, W, 3), dtype=F32, device=self.device)
            conf = torch.empty((B, H, W), dtype=F32, device=self.device)
        else:
            pts, conf = out
        if fused:
            L = self.w[p + ".head.2"]
            ops.conv3x3_dpt_final(o, L.w, L.b, self.w[p + ".head.4.w"], self.w[p + ".head.4.b"], pts, conf)
        else:
            ops.dpt_final(o.view(B * H * W, -1), self.w[p + ".head.4.w"], self.w[p + ".head.4.b"], 0, pts, conf)
        if res is not None:
            res[key_pts], res[key_conf] = pts, conf

    # ------------------------------------------------------------------ window forward
    @torch.no_grad()
    def forward_window(self, imgs: torch.Tensor, return_taps: bool = False):
        """imgs [V,3,H,W] on the GPU (fp32 normalised or uint8).  Returns (list of V pred dicts, taps).
        With graphs enabled the prediction tensors are static buffers, valid until the next call."""
        if self.use_graphs and not return_taps:
            with self._encoder_turn():       # the window graph holds an encoder pass
                return self._graphed("win", lambda x: self._forward_window(x, False), imgs.contiguous())
        return self._forward_window(imgs, return_taps)

    @torch.no_grad()
    def encode_batch(self, imgs: torch.Tensor) -> torch.Tensor:
        """encoder features fp32 [B,N,E] of B images (one batched pass; a fresh tensor the caller may keep)."""
        if self.use_graphs:
            with self._encoder_turn():
                feat, _, _ = self._graphed("enc", self._encode, imgs.contiguous())
                return feat.clone()
        return self._encode(imgs)[0]

    @torch.no_grad()
    def decode_window(self, feats: torch.Tensor, H: int, W: int):
        """Window inference from cached encoder features [V,N,E] (fp32): recurrent decoder + heads only.  The trackers
        keep every keyframe's features (keyframe.featI, hislam2/keyframe.py:36), so a keyframe is encoded ONCE instead
        of once in the filter and again in every window it belongs to ('double encoding')."""
        if self.use_graphs:
            return self._graphed(("dec", H, W), lambda f: self._forward_window(None, False, feats=f, hw=(H, W)), feats.contiguous())
        return self._forward_window(None, False, feats=feats, hw=(H, W))

    def _forward_window(self, imgs, return_taps: bool = False, feats=None, hw=None):
        """one window: images [V,3,H,W] (encoder + decoder + heads) or cached features [V,N,E] (decoder + heads)"""
        P = self.cfg.patch_size
        if feats is None:
            V, _, H, W = imgs.shape
            feat, feat16, _ = self._encode(imgs)
            res, taps = self._decode(feat[None], feat16[None], H, W, return_taps)
        else:
            H, W = hw
            res, taps = self._decode(feats[None], None, H, W, return_taps)
            V = feats.shape[0]
        preds = [{k: v[i:i + 1] for k, v in res.items()} for i in range(V)]
        return preds, taps

    @torch.no_grad()
    def decode_windows(self, feats: torch.Tensor, H: int, W: int):
        """Batched window inference: feats [Wn,V,N,E] fp32 (cached encoder features of Wn INDEPENDENT tracking windows:
        every window re-initialises state and pose memory, model.py:819-822) -> dict of stacked predictions
        (pts3d_in_self_view [Wn*V,H,W,3], conf_self [Wn*V,H,W], camera_pose [Wn*V,7], window-major).  The recurrent decoder
        is sequential over the V views but its GEMMs/attention are batched over the Wn windows (M = Wn*768 rows),
        which lifts them from the latency-bound tile-64 regime into the MFMA-bound tile-128 regime."""
        if self.use_graphs:
            return self._graphed(("decW", H, W), lambda f: self._decode(f, None, H, W, False)[0], feats.contiguous())
        return self._decode(feats, None, H, W, False)[0]

    def _decode(self, feat, feat16, H, W, return_taps=False):
        """feat fp32 [Wn,V,N,E] (+ optional fp16 copy).  Returns (dict of [Wn*V,...] tensors, taps)."""
        cfg = self.cfg
        P, E, D, Ld = cfg.patch_size, cfg.enc_embed_dim, cfg.dec_embed_dim, cfg.dec_depth
        Wn, V, N, _ = feat.shape
        nh, nw = H // P, W // P
        S = cfg.state_size
        dev = self.device
        if feat16 is None:
            feat16 = self.buf("win.feat16", (Wn, V, N, E), F16)
            ops.cast_f16(feat.reshape(Wn * V * N, E), feat16.view(Wn * V * N, E))
        y, xx = torch.meshgrid(torch.arange(nh, device=dev), torch.arange(nw, device=dev), indexing="ij")
        pos1 = torch.stack([y.reshape(-1), xx.reshape(-1)], -1)[None]                                  # [1,N,2]
        pos_img = torch.cat([-torch.ones(1, 1, 2, dtype=torch.int64, device=dev), pos1], dim=1).expand(Wn, -1, -1).contiguous()
        pos_state = self.state_pos.expand(Wn, -1, -1).contiguous()
        taps = {"enc_feat": feat[0]} if return_taps else None

        # a layer as pair launches (`pair_gemm`, or `pair_rows` at few rows) instead of one block per capture stream; what they carry: _pair_carries
        small = self._pair_carries(Wn * max(N + 1, S))
        pair = self.pair_gemm or small
        # LayerNorm fold: every residual buffer of the decoder has its fp16 copy + slab statistics, written by the GEMM that fills it
        fold = self.ln_fold and D % 64 == 0 and self._folded("dec_blocks.0.attn.qkv") and (small or not pair)

        def stream(name, rows):
            x = self.buf(name, (rows, D), F32)
            return _Stream(x, *self._xs(name, x)) if fold else _Stream(x)
        st = [stream("dec.state0", Wn * S), stream("dec.state1", Wn * S)]
        im = [stream("dec.img0", Wn * (N + 1)), stream("dec.img1", Wn * (N + 1))]
        # state init (model.py:538-568, 705-711): identical for every window
        s0 = self.buf("dec.s0", (S, D), F32)
        self._linear(self.register_tokens16, "decoder_embed_state", s0)
        st[0].x.view(Wn, S, D).copy_(s0[None].expand(Wn, -1, -1))
        msz = self.mem0.shape[0]
        mem = [self.buf("dec.mem0", (Wn * msz, 2 * D), F32), self.buf("dec.mem1", (Wn * msz, 2 * D), F32)]
        mem[0].view(Wn, msz, 2 * D).copy_(self.mem0[None].expand(Wn, -1, -1))
        h1, h2 = Ld * 2 // 4, Ld * 3 // 4
        tok1 = self.buf("head.tok1", (Wn, V, N, D), F16)
        tok2 = self.buf("head.tok2", (Wn, V, N, D), F16)
        tok3 = self.buf("head.tok3", (Wn, V, N, D), F16)
        tok3_32 = self.buf("head.tok3_32", (Wn, V, N, D), F32) if not self.minimal else None
        pose_tok = self.buf("head.pose_tok", (Wn, V, D), F32)
        pose_tok16 = self.buf("head.pose_tok16", (Wn, V, D), F16)
        g32 = self.buf("dec.g32", (Wn, E), F32)
        g16 = self.buf("dec.g16", (Wn, E), F16)
        if not self.one_key:
            dn32 = self.buf("dec.dn32", (Wn * (N + 1), D), F32)
            dn16 = self.buf("dec.dn16", (Wn * (N + 1), D), F16)
        Lde = self.w["decoder_embed"]
        w_de = Lde.w.unsqueeze(0).expand(Wn, -1, -1)
        b_de = Lde.b.unsqueeze(0).expand(Wn, -1)
        states = []
        cs, cm = 0, 0             # current state / mem buffer index
        fork = self.dual_stream and self.use_graphs and torch.cuda.is_current_stream_capturing()
        if fork and self._side is None:
            self._side = torch.cuda.Stream()
        head_fork = fork and self.head_overlap and cfg.head_type == "dpt"
        head_pts = head_conf = None
        if head_fork:
            if self._head_stream is None:
                self._head_stream = torch.cuda.Stream()
            head_pts = torch.empty((Wn * V, H, W, 3), dtype=F32, device=dev)
            head_conf = torch.empty((Wn * V, H, W), dtype=F32, device=dev)
        for i in range(V):
            ops.colmean_batched(feat[:, i], g32)                 # global feature of view i, every window, one launch
            ops.cast_f16(g32, g16)
            a, b = im[0], im[1]
            a3 = a.x.view(Wn, N + 1, D)
            if i == 0:
                a3[:, 0] = self.pose_token
            else:
                a3[:, 0] = self._mem_inquire(g16, mem[cm], Wn)
            ops.linear_batched(feat16[:, i], w_de, a3[:, 1:], b_de)                                   # decoder_embed
            s_a, s_b = st[cs], st[cs ^ 1]
            # after the window's last view the recurrent state and the pose memory are never read again (the next window
            # re-initialises both, model.py:819-822): their final updates are skipped unless the caller asked for them
            dead_tail = (i == V - 1) and not return_taps
            # LayerNorm fold: the first layer's inputs come from decoder_embed / the state carry (LayerNorm launches); from the second layer of
            # a view on they were written by the previous layer's fc2 together with their fp16 copies and slab statistics
            fresh = False
            for l in range(Ld):
                last = dead_tail and l == Ld - 1          # only the image block still feeds the heads
                pre = bool(not last and self.dual_ln and D in (768, 1024, 1536) and not (fold and fresh))
                if pre:
                    self._dual_norms(l, a.x, s_a.x)
                image = self._block(f"dec_blocks.{l}", "deci", a, s_a, b, pos_img, pos_state, cfg.dec_num_heads, Wn, fresh, pre)
                state = None if last else self._block(f"dec_blocks_state.{l}", "decs", s_a, a, s_b, pos_state, pos_img, cfg.state_dec_num_heads,
                                                      Wn, fresh, pre)
                if last:
                    self._dec_layer([image])
                elif pair:
                    self._dec_layer([state, image], fork)
                elif fork:
                    cur = torch.cuda.current_stream()
                    self._side.wait_stream(cur)
                    with torch.cuda.stream(self._side):
                        self._dec_layer([state])
                    self._dec_layer([image])
                    cur.wait_stream(self._side)
                else:
                    self._dec_layer([state])
                    self._dec_layer([image])
                s_a, s_b = s_b, s_a
                a, b = b, a
                fresh = True
                for tk, h in ((tok1, h1), (tok2, h2)):          # (a decoder of depth 2 taps the same layer twice)
                    if l + 1 == h:
                        tk[:, i].copy_(a.x.view(Wn, N + 1, D)[:, 1:])      # fp32 -> fp16 (round to nearest even), one strided copy
            # final norms (model.py:694-697): new state = dec_norm_state(state), img = dec_norm(img)
            if not dead_tail:
                self._ln(s_a.x, "dec_norm_state", out32=s_b.x)
            new_state = s_b
            if self.one_key:        # every row straight to where the heads and the pose memory read it
                ops.layernorm_tokens(a.x, *self.w["dec_norm"], cfg.ln_eps, pose_tok[:, i], pose_tok16[:, i], tok3[:, i],
                                     None if tok3_32 is None else tok3_32[:, i])
            else:
                self._ln(a.x, "dec_norm", out16=dn16, out32=dn32)
                dn16v, dn32v = dn16.view(Wn, N + 1, D), dn32.view(Wn, N + 1, D)
                tok3[:, i].copy_(dn16v[:, 1:])
                if tok3_32 is not None:
                    tok3_32[:, i].copy_(dn32v[:, 1:])
                pose_tok[:, i].copy_(dn32v[:, 0])
                pose_tok16[:, i].copy_(dn16v[:, 0])
            if not dead_tail:
                self._mem_update(mem[cm], g16, pose_tok[:, i], mem[cm ^ 1], Wn)
                cm ^= 1
            if head_fork:
                # fork: this view's DPT head (batch = the Wn windows) runs beside the decoder of the next view
                cur = torch.cuda.current_stream()
                self._head_stream.wait_stream(cur)
                with torch.cuda.stream(self._head_stream):
                    for c0 in range(0, Wn, self.head_chunk):
                        c1 = min(Wn, c0 + self.head_chunk)
                        nb = c1 - c0
                        tk = []
                        for name, src, dim in (("f", feat16, E), ("t1", tok1, D), ("t2", tok2, D), ("t3", tok3, D)):
                            if self.one_key:        # the 1 x 1 convolutions read view i of the windows where it lies (_conv1)
                                tk.append(src[c0:c1, i])
                                continue
                            t = self.buf("head.view." + name, (nb, N, dim), F16)
                            t.copy_(src[c0:c1, i])
                            tk.append(t.view(nb * N, dim))
                        pd, cd = head_pts.view(Wn, V, H, W, 3)[c0:c1, i], head_conf.view(Wn, V, H, W)[c0:c1, i]
                        if self._dpt_fused("downstream_head.dpt_self"):
                            # the fused output stage writes view i of windows c0..c1 in place (view stride = one window)
                            self._dpt_pts("downstream_head.dpt_self", tk, nb, nh, nw, H, W, None, None, None, out=(pd, cd))
                        else:
                            pv = self.buf("head.view.pts", (nb, H, W, 3), F32)
                            cv = self.buf("head.view.conf", (nb, H, W), F32)
                            self._dpt_pts("downstream_head.dpt_self", tk, nb, nh, nw, H, W, None, None, None, out=(pv, cv))
                            pd.copy_(pv)
                            cd.copy_(cv)
            # the state ping-pong: make st[cs] hold the new state for the next view
            cs = 0 if new_state is st[0] else 1
            if return_taps:
                states.append((new_state.x.view(Wn, S, D)[0].clone(), mem[cm].view(Wn, msz, 2 * D)[0].clone()))
        if return_taps:
            taps["states"] = states

        # ---- heads, batched over all Wn*V views
        BV = Wn * V
        h = "downstream_head"
        ph = self.buf("head.pose_h", (BV, self.w[h + ".pose_head.mlp.fc1"].npad), F16)
        self._linear(pose_tok16.view(BV, D), h + ".pose_head.mlp.fc1", ph, act=1)
        praw = self.buf("head.pose_raw", (BV, 8), F32)
        self._linear(ph, h + ".pose_head.mlp.fc2", praw)
        pose = torch.empty((BV, 7), dtype=F32, device=dev)
        ops.postprocess_pose(praw[:, :7].contiguous(), pose)
        res: Dict[str, torch.Tensor] = {"camera_pose": pose}
        toks = [feat16.reshape(BV * N, E), tok1.view(BV * N, D), tok2.view(BV * N, D), tok3.view(BV * N, D)]
        if head_fork:
            torch.cuda.current_stream().wait_stream(self._head_stream)          # join the head branch
            res["pts3d_in_self_view"], res["conf_self"] = head_pts, head_conf
        elif cfg.head_type == "dpt":
            # chunks of <= 8 views keep the implicit-GEMM grids (M/128 row tiles on grid.y) inside the 65535 limit
            pts = torch.empty((BV, H, W, 3), dtype=F32, device=dev)
            conf = torch.empty((BV, H, W), dtype=F32, device=dev)
            for c0 in range(0, BV, 8):
                c1 = min(BV, c0 + 8)
                tk = [t.view(BV, N, -1)[c0:c1].reshape((c1 - c0) * N, -1) for t in toks]
                self._dpt_pts(h + ".dpt_self", tk, c1 - c0, nh, nw, H, W, None, None, None, out=(pts[c0:c1], conf[c0:c1]))
            res["pts3d_in_self_view"], res["conf_self"] = pts, conf
        else:
            self._linear_head(h + ".proj", tok3.view(BV * N, D), BV, nh, nw, True, "pts3d_in_self_view", "conf_self", res)
        if not self.minimal:
            posBV = pos1.expand(BV, -1, -1).contiguous()
            self._cross_heads(toks, tok3_32.view(BV, N, D), pose_tok.view(BV, D), posBV, BV, nh, nw, H, W, res)
        return res, taps

    def _linear_head(self, p, tok16, V, nh, nw, pos_z, key_pts, key_conf, res, rgb=False):
        P = self.cfg.patch_size
        hdim = self.w[p + ".fc1"].npad
        hb = self.buf(p + ".h", (tok16.shape[0], hdim), F16)
        self._linear(tok16, p + ".fc1", hb, act=1)
        nout = self.w[p + ".fc2"].npad
        raw = self.buf(p + ".raw", (tok16.shape[0], nout), F32)
        self._linear(hb, p + ".fc2", raw)
        nch = nout // (P * P)
        # pixel shuffle: token (py,px), channel (c,iy,ix) -> pixel (py*P+iy, px*P+ix), channel c   (linear_head.py:310-313)
        fmap = raw.view(V, nh, nw, nch, P, P).permute(0, 1, 4, 2, 5, 3).reshape(V * nh * P * nw * P, nch).contiguous()
        H, W = nh * P, nw * P
        pts = torch.empty((V, H, W, 3), dtype=F32, device=self.device)
        if rgb:
            res[key_pts] = ((torch.sigmoid(fmap) * (1 - 2e-6) + 1e-6 - 0.5) * 2).view(V, H, W, 3)
            return
        conf = torch.empty((V, H, W), dtype=F32, device=self.device)
        ops.postprocess_pts(fmap, pos_z, pts, conf)
        res[key_pts], res[key_conf] = pts, conf

    def _cross_heads(self, toks, tok3_32, pose_tok, pos, V, nh, nw, H, W, res):
        """pts3d_in_other_view / conf / rgb (dpt_head.py:219-259, linear_head.py:299-346); not consumed by SLAM."""
        cfg = self.cfg
        h = "downstream_head"
        D, N = cfg.dec_embed_dim, nh * nw
        heads = cfg.dec_num_heads
        x = self.buf("ft.x", (V * N, D), F32)
        x.copy_(tok3_32.view(V * N, D))
        ln16 = self.buf("ft.ln16", (V * N, D), F16)
        mod = self.buf("ft.mod", (V, 2 * D), F32)
        for i in range(2):
            p = f"{h}.final_transform.{i}"
            for n, fn in (("norm1", "attn"), ("norm2", "mlp")):
                L = self.w[f"{p}.{n}.mlp.1"]
                ops.gemv(pose_tok, L.w, mod, L.b, silu_in=True)
                for v in range(V):            # modulation vectors are per view (batch element)
                    sh, sc = mod[v, :D].contiguous(), mod[v, D:].contiguous()
                    g, b = self.w[f"{p}.{n}.norm"]
                    ops.layernorm(x[v * N:(v + 1) * N], g, b, cfg.ln_eps, ln16[v * N:(v + 1) * N], None, sc, sh)
                if fn == "attn":
                    self._self_attn("ft", ln16, V, N, heads, pos, p + ".attn", x, x)
                else:
                    self._mlp("ft", ln16, p + ".mlp", x, x)
        tc16 = self.buf("ft.tc16", (V * N, D), F16)
        ops.cast_f16(x, tc16)
        if cfg.head_type == "dpt":
            if cfg.rgb_head:
                p = h + ".dpt_rgb"
                o = self._dpt(p, toks, V, nh, nw)
                rgb = torch.empty((V, H, W, 3), dtype=F32, device=self.device)
                ops.dpt_final(o.view(V * H * W, -1), self.w[p + ".head.4.w"], self.w[p + ".head.4.b"], 1, rgb, None)
                res["rgb"] = rgb
            self._dpt_pts(h + ".dpt_cross", toks[:3] + [tc16], V, nh, nw, H, W, "pts3d_in_other_view", "conf", res)
        else:
            if cfg.rgb_head:
                self._linear_head(h + ".rgb_proj", toks[3], V, nh, nw, False, "rgb", None, res, rgb=True)
            self._linear_head(h + ".cross_proj", tc16, V, nh, nw, False, "pts3d_in_other_view", "conf", res)

    # ------------------------------------------------------------------ reference-shaped entry points
    @torch.no_grad()
    def forward(self, views, ret_state=False):
        """views: list of view dicts (hislam2/track_frontend.py:51-72); only the SLAM mode is supported
        (img_mask=True, ray_mask=False, update=True, reset=False for every view, batch 1)."""
        for v in views:
            if v["img"].shape[0] != 1:
                raise NotImplementedError("batch size per view must be 1 (as in the SLAM trackers)")
            if not bool(v["img_mask"].all()) or bool(v["ray_mask"].any()) or bool(v["reset"].any()) or \
                    (v.get("update") is not None and not bool(v["update"].all())):
                raise NotImplementedError("only img_mask=True, ray_mask=False, update=True, reset=False is supported")
        imgs = torch.cat([v["img"] for v in views], 0).to(self.device, F32)
        preds, _ = self.forward_window(imgs)
        out = ARCroco3DStereoOutput(ress=preds, views=views)
        return (out, None) if ret_state else out

    __call__ = forward


# name aliases so `from cut3r_slam_amd.model import ARCroco3DStereo` reads like the reference import
ARCroco3DStereo = Cut3rModel


def _config_from_ctor_string(s: str, base: Cut3rConfig) -> Cut3rConfig:
    """Parse 'ARCroco3DStereo(ARCroco3DStereoConfig(state_size=768, ..., enc_embed_dim=1024, ...))' (the string the reference
    eval()s, model.py:72-92) without eval.  Output activations other than the ones this runtime implements --
    depth_mode ('exp', -inf, inf), conf_mode ('exp', 1, inf), pose_mode ('exp', -inf, inf) (heads/postprocess.py:11-63) -- and a
    checkpoint without pose head are refused instead of being silently mis-evaluated."""
    if not s:
        return base
    d = base.to_dict()
    for key in ("state_size", "local_mem_size", "enc_embed_dim", "enc_depth", "enc_num_heads", "dec_embed_dim",
                "dec_depth", "dec_num_heads", "state_dec_num_heads", "ray_enc_depth", "patch_size", "mlp_ratio"):
        m = re.search(rf"\b{key}\s*=\s*(\d+)", s)
        if m:
            d[key] = int(m.group(1))
    m = re.search(r"head_type\s*=\s*['\"](\w+)['\"]", s)
    if m:
        d["head_type"] = m.group(1)
    m = re.search(r"img_size\s*=\s*[\(\[]\s*(\d+)\s*,\s*(\d+)\s*[\)\]]", s)
    if m:
        d["img_size"] = (int(m.group(1)), int(m.group(2)))
    for key in ("rgb_head", "pose_head"):
        m = re.search(rf"\b{key}\s*=\s*(True|False)", s)
        if m:
            d[key] = m.group(1) == "True"
    m = re.search(r"pos_embed\s*=\s*['\"]RoPE(\d+(?:\.\d+)?)['\"]", s)
    if m:
        d["rope_freq"] = float(m.group(1))
    elif re.search(r"pos_embed\s*=", s):
        raise NotImplementedError("only RoPE position embeddings (pos_embed='RoPE<freq>') are implemented")
    want = {"depth_mode": ("exp", "-inf", "inf"), "conf_mode": ("exp", "1", "inf"), "pose_mode": ("exp", "-inf", "inf")}
    for key, exp in want.items():
        m = re.search(rf"\b{key}\s*=\s*[\(\[]\s*['\"](\w+)['\"]\s*,\s*([^,]+?)\s*,\s*([^\)\]]+?)\s*[\)\]]", s)
        if m:
            got = (m.group(1), m.group(2).replace("float('inf')", "inf").replace('float("inf")', "inf").replace("1.0", "1").replace(" ", ""),
                   m.group(3).replace("float('inf')", "inf").replace('float("inf")', "inf").replace(" ", ""))
            if got != exp:
                raise NotImplementedError(f"{key}={got}: this runtime implements {exp} only")
    if not d.get("pose_head", True):
        raise NotImplementedError("checkpoints without pose head are not supported (the SLAM trackers need camera_pose)")
    return Cut3rConfig.from_dict(d)
