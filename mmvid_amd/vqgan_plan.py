"""Planner of the op list that `mmvid_vqgan_run` (csrc/vqgan.hip) executes for one VQGAN encode / decode of a given batch shape.

`vae.py` mirrors the reference's classes; this module decides everything about execution: which kernel form every layer runs in,
which precisions it stores and where every tensor lives in the arena.  Its whole output is a flat array of `mmvid_vqgan_op_t` plus an
arena size (tests/test_vqgan_plan_pin.py pins both, per mode and shape).

* one planner class per operator -- `Bf16Planner` (the default: bf16 MFMA operands), `StrictPlanner` (fp32, csrc/strict.hip) and
  `PairPlanner` (bf16-pair convolutions, `vae.strict = 'split'`; with `f16_side` the fp16 layers of `'mixed'`).  `_Planner` holds what
  they share: the arena, the op records, the geometry rules of the convolution forms;
* `conv_weights`: the one re-layout of a conv holder's frozen weights, in the four encodings the operators read;
* `plan_encode` / `plan_decode`: the walk over the network (taming/modules/diffusionmodules/model.py), the same for every operator.

A sharp edge, kept on purpose: a planned tensor's arena range returns to the free list when the LAST PYTHON REFERENCE to its `_Buf`
drops (`_Buf.__del__`), so the lifetime of a local variable in this module is the liveness of a tensor on the device, and moving a
temporary into or out of a function moves offsets.  The pinned plans show any such change."""
import torch

from . import _lib, ops

bf16, f32 = torch.bfloat16, torch.float32

# The flags and op codes of mmvid_vqgan_op_t come from include/mmvid_hip.h, which says what each means and which go together (bits
# 1, 2 and 8 mean one thing on a CONV and another on a GROUPNORM).  A name the header lacks is a KeyError here, at import.
FLAG_NAMES = ('RES_F32', 'IN_F32', 'CLAMP01', 'STATS_GIVEN', 'EMIT_STATS', 'STRIP', 'BLOCKS64', 'STRICT', 'SPLITK', 'SPLIT', 'F16')
RES_F32, IN_F32, CLAMP01, STATS_GIVEN, EMIT_STATS, STRIP, BLOCKS64, STRICT, SPLITK, SPLIT, F16 = (
    _lib.HEADER.constants['MMVID_VQFLAG_' + name] for name in FLAG_NAMES)
OP_NAMES = {'OP_IMG': 'IMG2NHWC8', 'OP_CONV': 'CONV', 'OP_GN': 'GROUPNORM', 'OP_CAST': 'CAST', 'OP_ATTN': 'SPATIAL_ATTN',
            'OP_VQ': 'VQ_ARGMIN', 'OP_GATHER': 'GATHER', 'OP_NCHW': 'NHWC2NCHW', 'OP_EXT': 'EXT_CAST'}  # the planner's name -> the header's


def _pow2_at_least8(c):
    p = 8
    while p < c:
        p *= 2
    return p


def conv_weights(holder, form):
    """conv holder -> (w [Cout_p, taps, Cin_p], bias f32 [Cout_p], Cout): the weights permuted to [Cout][ky][kx][Cin] and zero-padded, as
    'bf16' | 'f16' | 'pair' (bf16 [Cout_p, 3, taps, Cin_p] = (w_hi | w_hi | w_lo) with w_hi = bf16(w), w_lo = bf16(w - w_hi)) |
    'f32' (the strict operator: Cin padded to 4 or a power of two, Cout not at all)."""
    w, b = holder.weight.detach().float(), holder.bias.detach().float()
    cout, cin, kh, kw = w.shape
    if form == 'f32':
        cin_p, cout_p = (4 if cin <= 4 else _pow2_at_least8(cin)), cout
    else:
        cin_p, cout_p = _pow2_at_least8(cin), (cout + 7) // 8 * 8
    wp = torch.zeros(cout_p, kh * kw, cin_p, device=w.device, dtype=f32)
    wp[:cout, :, :cin] = w.permute(0, 2, 3, 1).reshape(cout, kh * kw, cin)
    bp = torch.zeros(cout_p, device=w.device, dtype=f32)
    bp[:cout] = b
    if form == 'pair':
        hi = wp.to(bf16)
        wp = torch.stack([hi, hi, (wp - hi.float()).to(bf16)], 1)
    elif form != 'f32':
        wp = wp.to({'bf16': bf16, 'f16': torch.float16}[form])
    return wp.contiguous(), bp, cout


class _Buf:
    """Planned tensor: a byte range of the arena.  Dropping the last reference returns the range to the planner's
    free list, which is exactly the liveness rule a single in-order stream needs."""

    def __init__(self, pl, off, nbytes, shape, dtype):
        self.pl, self.off, self.nbytes, self.shape, self.dtype = pl, off, nbytes, shape, dtype

    def __del__(self):
        if self.pl is not None and self.pl.recording:
            self.pl.free.append((self.off, self.nbytes))


class _Plan:
    def __init__(self, ops_arr, arena, patches, kept):
        self.ops, self.arena, self.patches, self.kept = ops_arr, arena, patches, kept

    def run(self, ext_in, ext_out):
        for i, field, name in self.patches:
            src = ext_in if field == 'ext_in' else ext_out
            setattr(self.ops[i], field, src[name].data_ptr())
        _lib.call('mmvid_vqgan_run', self.ops, len(self.ops), ops._p(self.arena), ops._stream())


class _Planner:
    """What the three operators share.  An operator implements image, conv, gn, cast, attn_block, gather and external_z."""
    OP_IMG, OP_CONV, OP_GN, OP_CAST, OP_ATTN, OP_VQ, OP_GATHER, OP_NCHW, OP_EXT = (
        _lib.HEADER.constants['MMVID_VQOP_' + name] for name in OP_NAMES.values())
    STRICT, SPLIT, F16 = STRICT, SPLIT, F16
    strict = split = False  # which operator this is, for readers of a planner; no method branches on them

    def __init__(self, vae):
        self.vae, self.ops, self.free, self.top, self.recording = vae, [], [], 0, True
        self.patches, self.kept, self._pinned = [], {}, []

    # arena allocation: first fit in the free list, else bump
    def alloc(self, shape, dtype):
        n = 1
        for d in shape:
            n *= d
        nbytes = (n * (2 if dtype == bf16 else 4) + 255) // 256 * 256
        for i, (off, sz) in enumerate(self.free):
            if sz >= nbytes:
                if sz > nbytes:
                    self.free[i] = (off + nbytes, sz - nbytes)
                else:
                    self.free.pop(i)
                return _Buf(self, off, nbytes, tuple(shape), dtype)
        off = self.top
        self.top += nbytes
        return _Buf(self, off, nbytes, tuple(shape), dtype)

    def _op(self, patch=None, **kw):
        """Append one op; patch = (field, name): the external pointer that _Plan.run fills in on every call."""
        o = _lib.VqganOp()
        o.in0 = o.in1 = o.in2 = o.out_bf16 = o.out_f32 = o.scratch = -1
        for k, v in kw.items():
            setattr(o, k, v)
        self.ops.append(o)
        if patch is not None:
            self.patches.append((len(self.ops) - 1, ) + patch)
        return o

    # ---- the geometry rules of the convolution forms (the bf16 and the pair operator; geometry only, like every kernel choice) -------
    @staticmethod
    def _out_hw(h, wd, mode):  # mode 1: Downsample (stride 2), 2: Upsample (nearest x2 + conv), 0 / 3: 3x3 / 1x1 at the input's size
        return (h // 2, wd // 2) if mode == 1 else ((2 * h, 2 * wd) if mode == 2 else (h, wd))

    @staticmethod
    def _strip(mode, clamp01, h, wd, cin, cout):
        """3x3 stride-1 layers at 32x32 and above run in strip form (csrc/conv_strip.hip)."""
        return mode == 0 and not clamp01 and bool(_lib.load().mmvid_conv3x3_strip_supported(h, wd, cin, cout))

    def _conv_scratch(self, out, feeds_gn, strip, mode, n, ho, wo, cin, cout):
        """What a convolution does with its `scratch` -> (flags, offset, the workspace to hold until the op is recorded).
        feeds_gn: a GroupNorm reads `out` next -> the epilogue also emits its partial statistics (when the shape allows), into a stats
        area that lives as long as `out`.  Otherwise a deep 3x3 layer on an 8x8 map, whose 128x128 output tiles alone cover a fraction
        of the chip, runs split-K by 4 through an fp32 workspace."""
        if feeds_gn and (ho * wo) % 128 == 0 and cout % 128 == 0:
            out.gn_stats = self._gn_stats(n, ho * wo, cout)
            out.gn_stats.blocks64 = strip
            return EMIT_STATS, out.gn_stats.off, None
        if not strip and mode == 0 and ho * wo <= 64 and 9 * cin >= 2304 and cout % 4 == 0:
            ws = self.alloc((4 * n * ho * wo * cout, ), f32)
            return SPLITK, ws.off, ws
        return 0, -1, None

    def _gn_stats(self, n, hw, c):
        return self.alloc((ops.gn_stats_floats(n, hw, c), ), f32)

    def _gn_given_stats(self, x):
        """The stats area of a GroupNorm that reads x and its flags: partial sums already written by the producing convolution's
        epilogue, else an area of its own."""
        st = getattr(x, 'gn_stats', None)
        if st is None:
            n, h, wd, c = x.shape
            return self._gn_stats(n, h * wd, c), 0
        return st, STATS_GIVEN | (BLOCKS64 if st.blocks64 else 0)

    def vq_argmin(self, z):
        n, h, wd, c = z.shape
        cb = self.vae.model.quantize.embedding.weight
        self._op(('ext_out', 'idx'), op=self.OP_VQ, N=n, H=h, W=wd, C=c, Cout=cb.shape[0], in0=z.off, w=cb.data_ptr(),
                 b=self.vae._ee().data_ptr())

    def to_nchw(self, x, cuse):
        n, h, wd, c = x.shape
        self._op(('ext_out', 'img'), op=self.OP_NCHW, N=n, H=h, W=wd, C=c, Cout=cuse, in0=x.off)

    def keep(self, name, buf):
        """Pin a planned tensor so it can be read back after run() (tests / encode_z)."""
        self.kept[name] = (buf.off, buf.shape)
        self._pinned.append(buf)

    def finish(self, device):
        self.recording = False
        arr = (_lib.VqganOp * len(self.ops))(*self.ops)
        arena = torch.empty(max(self.top, 256), device=device, dtype=torch.uint8)
        return _Plan(arr, arena, self.patches, self.kept)


class Bf16Planner(_Planner):
    """The default operator: every conv input bf16 (MFMA, fp32 accumulate), GroupNorm statistics fp32.  stream16: the residual stream
    between blocks is stored as bf16 as well (no fp32 activation leaves a conv except the VQ rows and the decoded image)."""

    def __init__(self, vae, stream16=False):
        super().__init__(vae)
        self.stream16 = bool(stream16)

    def image(self, n, s):
        out = self.alloc((n, s, s, 8), bf16)
        self._op(('ext_in', 'img'), op=self.OP_IMG, N=n, H=s, W=s, C=3, out_bf16=out.off)
        return out

    def conv(self, x, holder, mode, residual=None, out32=False, clamp01=False, feeds_gn=False, also_bf16=False, keep32=False):
        """feeds_gn: see _conv_scratch.  also_bf16 (with out32): the epilogue stores a bf16 copy too (`out.bf16`), instead of a later
        cast pass.  keep32: fp32 output even with a bf16 residual stream (the VQ rows, the decoded image)."""
        if self.stream16 and not keep32:
            out32 = also_bf16 = False
        w, b, _ = self.vae._cw(holder, 'bf16')
        n, h, wd, cin = x.shape
        assert x.dtype == bf16 and cin == w.shape[2], (x.shape, w.shape)
        ho, wo = self._out_hw(h, wd, mode)
        cout = w.shape[0]
        out = self.alloc((n, ho, wo, cout), f32 if out32 else bf16)
        strip = self._strip(mode, clamp01, h, wd, cin, cout)
        sflags, scratch, ws = self._conv_scratch(out, feeds_gn, strip, mode, n, ho, wo, cin, cout)
        flags = (RES_F32 if (residual is not None and residual.dtype == f32) else 0) | (CLAMP01 if clamp01 else 0) | \
            (STRIP if strip else 0) | sflags
        o16 = out.off if not out32 else -1
        if out32 and also_bf16:
            out.bf16 = self.alloc((n, ho, wo, cout), bf16)
            o16 = out.bf16.off
        self._op(op=self.OP_CONV, mode=mode, N=n, H=h, W=wd, C=cin, Cout=cout, flags=flags, in0=x.off,
                 in1=residual.off if residual is not None else -1, out_bf16=o16,
                 out_f32=out.off if out32 else -1, scratch=scratch, w=w.data_ptr(), b=b.data_ptr())
        del ws  # the workspace returns to the free list: later tensors of the plan may reuse it (one in-order stream)
        return out

    def gn(self, x, holder, swish=True):
        n, h, wd, c = x.shape
        out = self.alloc(x.shape, bf16)
        st, flags = self._gn_given_stats(x)
        self._op(op=self.OP_GN, mode=int(swish), N=n, H=h, W=wd, C=c, flags=flags | (IN_F32 if x.dtype == f32 else 0), in0=x.off,
                 out_bf16=out.off, scratch=st.off, w=holder.weight.data_ptr(), b=holder.bias.data_ptr(), eps=1e-6)
        return out

    def cast(self, x):
        if x.dtype == bf16:
            return x
        if getattr(x, 'bf16', None) is not None:  # the producing conv already stored the bf16 copy
            return x.bf16
        out = self.alloc(x.shape, bf16)
        n, h, wd, c = x.shape
        self._op(op=self.OP_CAST, N=n, H=h, W=wd, C=c, in0=x.off, out_bf16=out.off)
        return out

    def attn_block(self, x32, blk, final='f32'):
        """model.py:180-205.  q / k / v (model.py:159-178: three 1x1 convs of the same input) are ONE 1x1 conv with the three weights
        stacked along Cout: one launch instead of three small ones; q, k, v are the column blocks of its [n, h, w, 3c] output."""
        h = self.gn(x32, blk.norm, swish=False)
        w, b = self.vae._cw_qkv(blk)
        n, ht, wd, cin = h.shape
        c, hw = w.shape[0] // 3, ht * wd
        qkv = self.alloc((n, ht, wd, 3 * c), bf16)
        self._op(op=self.OP_CONV, mode=3, N=n, H=ht, W=wd, C=cin, Cout=3 * c, flags=0, in0=h.off, out_bf16=qkv.off,
                 w=w.data_ptr(), b=b.data_ptr())
        o = self.alloc((n, ht, wd, c), bf16)
        sc = self.alloc((n * hw * hw * 3 // 2 + 64, ), f32)
        self._op(op=self.OP_ATTN, N=n, H=ht, W=wd, C=c, in0=qkv.off, in1=qkv.off + 2 * c, in2=qkv.off + 4 * c, out_bf16=o.off,
                 scratch=sc.off, eps=float(c)**-0.5, pad=3 * c)
        del sc
        out = self.conv(o, blk.proj_out, 3, residual=x32, out32=final != 'bf16', feeds_gn=final != 'bf16', also_bf16=final == 'both')
        del h, qkv, o  # (the order in which the ranges return to the free list is part of the plan)
        return out

    def gather(self, n, hw):
        cb = self.vae.model.quantize.embedding.weight
        out = self.alloc((n, hw, hw, cb.shape[1]), bf16)
        self._op(('ext_in', 'idx'), op=self.OP_GATHER, N=n, H=hw, W=hw, C=cb.shape[1], Cout=cb.shape[0], w=cb.data_ptr(),
                 flags=0, out_bf16=out.off)
        return out

    def external_z(self, n, hw, c):
        """decode_train: z [n*hw*hw, c] fp32 computed outside the plan (probs @ codebook) enters here."""
        out = self.alloc((n, hw, hw, c), bf16)
        self._op(('ext_in', 'z'), op=self.OP_EXT, N=n, H=hw, W=hw, C=c, flags=0, out_bf16=out.off)
        return out


class _Fp32StreamPlanner(_Planner):
    """What the two exact operators share: the tensors that enter a decode, and the attention, are fp32 (flag STRICT)."""

    def attn_block(self, x32, blk, final='f32'):
        """model.py:180-205, with the fp32 attention of csrc/strict.hip (for the pair operator it is 0.2 % of the encoder's work)."""
        h = self.gn(x32, blk.norm, swish=False)
        q, k, v = self.conv(h, blk.q, 3), self.conv(h, blk.k, 3), self.conv(h, blk.v, 3)
        n, ht, wd, c = q.shape
        hw = ht * wd
        o = self.alloc(q.shape, f32)
        sc = self.alloc((2 * n * hw * hw, ), f32)
        self._op(op=self.OP_ATTN, N=n, H=ht, W=wd, C=c, flags=STRICT, in0=q.off, in1=k.off, in2=v.off,
                 out_f32=o.off, scratch=sc.off, eps=float(c)**-0.5)
        del sc
        out = self.conv(o, blk.proj_out, 3, residual=x32, out32=final != 'bf16', feeds_gn=final != 'bf16')
        del h, o, q, k, v  # (the order in which the ranges return to the free list is part of the plan)
        return out

    def gather(self, n, hw):
        cb = self.vae.model.quantize.embedding.weight
        out = self.alloc((n, hw, hw, cb.shape[1]), f32)
        self._op(('ext_in', 'idx'), op=self.OP_GATHER, N=n, H=hw, W=hw, C=cb.shape[1], Cout=cb.shape[0], w=cb.data_ptr(),
                 flags=STRICT, out_f32=out.off)
        return out

    def external_z(self, n, hw, c):
        """decode_train: z [n*hw*hw, c] fp32 computed outside the plan (probs @ codebook) enters here."""
        out = self.alloc((n, hw, hw, c), f32)
        self._op(('ext_in', 'z'), op=self.OP_EXT, N=n, H=hw, W=hw, C=c, flags=STRICT, out_f32=out.off)
        return out


class StrictPlanner(_Fp32StreamPlanner):
    """vae.strict = True: the fp32 operator (csrc/strict.hip: f32 MFMA, fp64 GroupNorm statistics); every planned tensor is fp32."""
    strict = True

    def image(self, n, s):
        out = self.alloc((n, s, s, 4), f32)
        self._op(('ext_in', 'img'), op=self.OP_IMG, N=n, H=s, W=s, C=3, out_f32=out.off, flags=STRICT)
        return out

    def conv(self, x, holder, mode, residual=None, clamp01=False, **unused):
        w, b, _ = self.vae._cw(holder, 'f32')
        n, h, wd, cin = x.shape
        assert x.dtype == f32 and cin == w.shape[2], (x.shape, w.shape)
        ho, wo = self._out_hw(h, wd, mode)
        cout = w.shape[0]
        out = self.alloc((n, ho, wo, cout), f32)
        self._op(op=self.OP_CONV, mode=mode, N=n, H=h, W=wd, C=cin, Cout=cout, flags=STRICT | (CLAMP01 if clamp01 else 0), in0=x.off,
                 in1=residual.off if residual is not None else -1, out_f32=out.off, w=w.data_ptr(), b=b.data_ptr())
        return out

    def gn(self, x, holder, swish=True):
        n, h, wd, c = x.shape
        out = self.alloc(x.shape, f32)
        st = self.alloc((n * 2 * c, ), f32)
        self._op(op=self.OP_GN, mode=int(swish), N=n, H=h, W=wd, C=c, flags=STRICT, in0=x.off, out_f32=out.off,
                 scratch=st.off, w=holder.weight.data_ptr(), b=holder.bias.data_ptr(), eps=1e-6)
        return out

    def cast(self, x):
        return x


class _GnPlane:
    """'mixed' only: how the output of a planned pair-operator GroupNorm is encoded.  Its FIRST reader decides: a convolution that
    runs in the fp16 form switches the GroupNorm op to one fp16 plane (the first plane of the same buffer), any other reader fixes it
    as (hi, lo) bf16 planes."""

    def __init__(self, op):
        self.op, self.form = op, None

    def read_as_f16(self, f16_ok):
        """A convolution reads the buffer; f16_ok: it could run in the fp16 form.  -> whether it reads an fp16 plane."""
        if self.form is None:
            self.form = 'f16' if f16_ok else 'pair'
            if f16_ok:
                self.op.flags |= F16
        assert self.form == 'pair' or f16_ok, 'a GroupNorm output switched to fp16 has a second reader that needs bf16 pairs'
        return self.form == 'f16'


class PairPlanner(_Fp32StreamPlanner):
    """vae.strict = 'split': fp32 tensors between ops, every conv input a bf16 pair (3 products per convolution, fp32 accumulate).
    f16_side ('mixed'): 3x3 stride-1 convolutions on maps of at least f16_side x f16_side pixels that read a GroupNorm output run as
    ONE product of fp16 operands; 0 = every convolution is the bf16-pair operator."""
    split = True

    def __init__(self, vae, f16_side=0):
        super().__init__(vae)
        self.f16_side = int(f16_side)

    def _alloc_planes(self, n, h, wd, c):
        out = self.alloc((2, n, h, wd, c), bf16)
        out.is_planes, out.shape = True, (n, h, wd, c)
        return out

    def image(self, n, s):
        out = self._alloc_planes(n, s, s, 8)
        self._op(('ext_in', 'img'), op=self.OP_IMG, N=n, H=s, W=s, C=3, out_bf16=out.off, flags=SPLIT)
        return out

    def cast(self, x):
        """fp32 tensor -> pair planes (a no-op for a tensor that already is one)."""
        if getattr(x, 'is_planes', False):
            return x
        n, h, wd, c = x.shape
        assert x.dtype == f32 and c % 8 == 0, x.shape
        out = self._alloc_planes(n, h, wd, c)
        self._op(op=self.OP_CAST, N=n, H=h, W=wd, C=c, flags=SPLIT, in0=x.off, out_bf16=out.off)
        return out

    def conv(self, x, holder, mode, residual=None, out32=False, clamp01=False, feeds_gn=False, keep32=False, **unused):
        x = self.cast(x)
        n, h, wd, cin = x.shape
        cout = (holder.weight.shape[0] + 7) // 8 * 8
        ho, wo = self._out_hw(h, wd, mode)
        assert residual is None or residual.dtype == f32
        strip = self._strip(mode, clamp01, h, wd, cin, cout)
        # the result's only reader is another pair-operator convolution (a level's last tensor in front of its Downsample): the strip
        # kernel's epilogue stores the bf16 pair itself -- no fp32 store, no cast pass (the same planes bit for bit)
        planes_only = not out32 and not keep32 and strip and not feeds_gn
        out = self._alloc_planes(n, ho, wo, cout) if planes_only else self.alloc((n, ho, wo, cout), f32)
        gn = getattr(x, 'gn', None)
        f16_ok = bool(strip and self.f16_side and min(h, wd) >= self.f16_side and holder.weight.shape[2] == 3)
        f16 = gn.read_as_f16(f16_ok) if gn is not None else False
        w, b, _ = self.vae._cw(holder, 'f16' if f16 else 'pair')
        assert cin == w.shape[-1] and cout == w.shape[0], (x.shape, w.shape)
        sflags, scratch, ws = self._conv_scratch(out, feeds_gn, strip, mode, n, ho, wo, cin, cout)
        flags = SPLIT | (CLAMP01 if clamp01 else 0) | (STRIP if strip else 0) | (F16 if f16 else 0) | sflags
        self._op(op=self.OP_CONV, mode=mode, N=n, H=h, W=wd, C=cin, Cout=cout, flags=flags, in0=x.off,
                 in1=residual.off if residual is not None else -1, out_f32=-1 if planes_only else out.off,
                 out_bf16=out.off if planes_only else -1, scratch=scratch, w=w.data_ptr(), b=b.data_ptr())
        del ws
        return out

    def gn(self, x, holder, swish=True):
        n, h, wd, c = x.shape
        out = self._alloc_planes(n, h, wd, c)
        st, flags = self._gn_given_stats(x)
        op = self._op(op=self.OP_GN, mode=int(swish), N=n, H=h, W=wd, C=c, flags=SPLIT | flags, in0=x.off, out_bf16=out.off,
                      scratch=st.off, w=holder.weight.data_ptr(), b=holder.bias.data_ptr(), eps=1e-6)
        out.gn = _GnPlane(op)
        return out


# ---- the walk over the network: the op sequence of one encode / decode, for whichever operator `pl` is --------------------------------
def plan_resblock(pl, x32, blk, final='f32'):
    """model.py:130-150 on an fp32 residual stream.  final: 'f32' (residual stream continues), 'both' (a conv reads
    the result next as well) or 'bf16' (ONLY a conv reads it: no fp32 store at all)."""
    h = pl.conv(pl.gn(x32, blk.norm1), blk.conv1, 0, feeds_gn=True)
    h = pl.gn(h, blk.norm2)
    skip = x32
    if hasattr(blk, 'nin_shortcut'):
        skip = pl.conv(pl.cast(x32), blk.nin_shortcut, 3, out32=True)
    return pl.conv(h, blk.conv2, 0, residual=skip, out32=final != 'bf16', feeds_gn=final != 'bf16',
                   also_bf16=final == 'both')


def plan_encode(pl, model, n, s):
    """Encoder.forward (model.py:439-466) + quant_conv (vqgan.py:67-68) + VQ lookup (quantize.py:302-310)."""
    enc = model.encoder

    def needs_bf16(blk):  # a resblock whose shortcut is a 1x1 conv reads its input in bf16 too
        return hasattr(blk, 'nin_shortcut')

    h = pl.conv(pl.image(n, s), enc.conv_in, 0, out32=True, feeds_gn=True, also_bf16=needs_bf16(enc.down[0].block[0]))
    for li, d in enumerate(enc.down):
        has_down = hasattr(d, 'downsample')
        nxt = enc.down[li + 1].block[0] if li + 1 < len(enc.down) else enc.mid.block_1
        for bi, blk in enumerate(d.block):
            last = bi == len(d.block) - 1
            with_attn = len(d.attn) > 0
            # what the level's last tensor feeds: only the downsample conv (bf16) / the next block's shortcut too
            end = 'bf16' if has_down else ('both' if needs_bf16(nxt) else 'f32')
            mid = 'both' if (not last and needs_bf16(d.block[bi + 1])) else 'f32'
            want = end if last else mid
            h = plan_resblock(pl, h, blk, final='f32' if with_attn else want)
            if with_attn:
                h = pl.attn_block(h, d.attn[bi], final=want)
        if has_down:
            h = pl.conv(pl.cast(h), d.downsample.conv, 1, out32=True, feeds_gn=True, also_bf16=needs_bf16(nxt))
    h = plan_resblock(pl, h, enc.mid.block_1)
    h = pl.attn_block(h, enc.mid.attn_1)
    h = plan_resblock(pl, h, enc.mid.block_2)
    h = pl.conv(pl.gn(h, enc.norm_out), enc.conv_out, 0)
    z = pl.conv(h, model.quant_conv, 3, out32=True, keep32=True)  # [N, h, w, embed_dim] fp32 = VQ rows
    pl.keep('z', z)
    pl.vq_argmin(z)


def plan_decode(pl, model, n, hw, from_z=False):
    """codebook gather (vae.py:50) + post_quant_conv + Decoder.forward (model.py:551-582) + vae.py:55.
    from_z: the quantised map arrives as an external fp32 tensor instead (decode_train, vae.py:58-68)."""
    dec = model.decoder
    z0 = pl.external_z(n, hw, model.quantize.embedding.weight.shape[1]) if from_z else pl.gather(n, hw)
    h = pl.conv(z0, model.post_quant_conv, 3)
    h = pl.conv(h, dec.conv_in, 0, out32=True, feeds_gn=True)
    h = plan_resblock(pl, h, dec.mid.block_1)
    h = pl.attn_block(h, dec.mid.attn_1)
    h = plan_resblock(pl, h, dec.mid.block_2)
    for lvl in reversed(range(len(dec.up))):
        u = dec.up[lvl]
        for bi, blk in enumerate(u.block):
            h = plan_resblock(pl, h, blk)
            if len(u.attn) > 0:
                h = pl.attn_block(h, u.attn[bi])
        if hasattr(u, 'upsample'):
            h = pl.conv(pl.cast(h), u.upsample.conv, 2, out32=True, feeds_gn=True)
    h = pl.gn(h, dec.norm_out)
    img = pl.conv(h, dec.conv_out, 0, out32=True, clamp01=True, keep32=True)  # (clamp(x,-1,1)+1)/2 fused, vae.py:55
    pl.to_nchw(img, 3)
