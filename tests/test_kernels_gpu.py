"""GPU: EVERY launch of a forward against torch fp32 on the operands that launch really read (per-kernel oracle tests).

The whole-network goldens (tests/test_hrnet_gpu.py) pin the fp32 engine to the reference capture; the bf16 / fp8 engines run
DIFFERENT kernels (two-team conv_tt in bf16 and e4m3, the fused 48-channel BasicBlock, the restructured head32, generic
stride-2 / 1x1 variants, upsample_add) that a drift bound over 300 layers cannot check at tap resolution.  Here the plan's
taps (sncal_hrnet_plan_tap, include/sncal.h) copy the input / residual / output tensors of every op out of the workspace
while a REAL forward runs -- grouped launches, stacked frames, partial tiles, sub-batch of B frames as they are -- and each op
is recomputed with torch (fp32 conv2d / index arithmetic) from the SAME rounded operands:

    conv (+BN shift, +residual, ReLU)       hrnet.py:42-58, 79-99, 195-214, 357-391    all kernels that serve it
    fused BasicBlock (48 channels)          hrnet.py:42-58                              bblock48: conv1 -> bf16 -> conv2 + x
    fuse sums (1x1 + bilinear up, add)      hrnet.py:229-244                            upsample_add
    head (upsample, concat, 1x1, 1x1)       hrnet.py:316-329, 489-510                   head32 / head_fused, restructured
    e4m3 convolutions (C5)                  same layers, per-tensor / per-channel scales conv_tt<fp8>, its bf16 and e4m3 outputs

Tolerance = one ulp of the output type (bf16: 2^-7 |y|, the worst-case ulp of a value; e4m3: 2^-3 |y| + one subnormal step)
plus 1e-3 of fp32 accumulation-order slack -- a wrong tap, a wrong tile-edge pixel, a row of the neighbouring frame or a
mis-scaled channel is two orders of magnitude above it.

Between the launches (producer_reader_identity, run by every case on the same taps): a launch recomputed from the operands it READ is
correct on clobbered operands too, so the tap of every tensor and twin at its producing op must equal, byte for byte, the tap of the same
tensor at every later op that reads it.

The operand a reduced-precision launch reads is a TWIN (e4m3 codes, [16 hi | 16 lo] split codes), and the references above are built from
the twin itself; twin_value_identity (every case, same taps) holds each twin to the dense tensor it stands for, bit for bit: the helpers
of quant.hip that make twins in front of a launch, and the epilogues that write a twin beside the dense output.
"""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BN_EPS = 1e-5


# ---- reference-side weights: the fold of hrnet.py's load_state_dict, restated (fp64 fold, fp32 storage) ---------------------
X3_T = torch.float16          # 16-bit type of the split twins: the build's (sncal_x3_name()); set in run_case
# split-arithmetic slack as a fraction of sum |x w|: fp16 splits drop ~2^-22 of a product (measured worst case 1.1e-6 of sum |x w|,
# the fp32 accumulation itself), bf16 splits ~2^-16 (measured below 1e-5)
X3_SLACK = 2e-6


def folded(sd, name, bn, has_bias):
    w = sd[name + '.weight'].to(torch.float64)
    cout = w.shape[0]
    b = sd[name + '.bias'].to(torch.float64) if has_bias else torch.zeros(cout, dtype=torch.float64)
    if bn:
        g, beta = sd[bn + '.weight'].to(torch.float64), sd[bn + '.bias'].to(torch.float64)
        mu, var = sd[bn + '.running_mean'].to(torch.float64), sd[bn + '.running_var'].to(torch.float64)
        scale = g / torch.sqrt(var + BN_EPS)
        shift = beta + (b - mu) * scale
    else:
        scale, shift = torch.ones(cout, dtype=torch.float64), b
    return w.to(torch.float32), scale.to(torch.float32), shift.to(torch.float32)


class Weights:
    def __init__(self, net, sd, dev):
        self.units = {u[0]: u for u in net.conv_units()}
        self.sd, self.dev = sd, dev
        self.cache = {}

    def get(self, op):
        """(w_scaled fp32 (cout,cin,k,k) = w * BN scale in fp32 -- what the packers round --, shift fp32 (cout))."""
        name = op['name']
        if name in self.cache:
            return self.cache[name]
        if name in self.units:
            _, bn, cin, cout, k, stride, has_bias = self.units[name]
            w, sc, sh = folded(self.sd, name, bn, has_bias)
            ws = w * sc[:, None, None, None]
        else:                                   # head-internal slice of last_layer.0: columns col_off.., BN scale folded, no shift
            _, bn, cin0, cout0, _, _, has_bias = self.units['model.last_layer.0']
            w, sc, _ = folded(self.sd, 'model.last_layer.0', bn, has_bias)
            ws = torch.zeros((op['cout'], op['cin'], 1, 1), dtype=torch.float32)
            ws[:cout0] = w[:, op['col_off']:op['col_off'] + op['cin']] * sc[:, None, None, None]
            sh = torch.zeros(op['cout'], dtype=torch.float32)
            if name == 'headx.d':               # split head (fp32 engine): the direct tensor's product carries last_layer.0's shift
                sh[:cout0] = folded(self.sd, 'model.last_layer.0', bn, has_bias)[2]
        out = (ws.to(self.dev), sh.to(self.dev))
        self.cache[name] = out
        return out


def bf16r(t):
    return t.to(torch.bfloat16).to(torch.float32)


def e4m3_decode(u8):
    return u8.view(torch.float8_e4m3fn).to(torch.float32)


def e4m3_round(t):
    return t.clamp(-448.0, 448.0).to(torch.float8_e4m3fn).to(torch.float32)


def nchw(t):            # (N,H,W,C) any dtype -> (N,C,H,W) fp32
    return t.to(torch.float32).permute(0, 3, 1, 2).contiguous()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def conv_ref(x_nchw, w, stride):
    k = w.shape[-1]
    return F.conv2d(x_nchw, w, None, stride=stride, padding=k // 2)


def lerp_tables(out_size, in_size, dev):
    """ops.hip lerp_idx / head32.hip: PyTorch's align_corners=True index in fp32.  Returns i0, i1 (long), w0, w1 (fp32)."""
    scale = (torch.tensor(float(in_size - 1), dtype=torch.float32) / torch.tensor(float(out_size - 1), dtype=torch.float32)) \
        if out_size > 1 else torch.tensor(0.0, dtype=torch.float32)
    o = torch.arange(out_size, dtype=torch.float32)
    src = scale * o
    i0 = src.to(torch.int64).clamp(max=in_size - 1)
    i1 = i0 + (i0 < in_size - 1).to(torch.int64)
    w1 = src - i0.to(torch.float32)
    w0 = 1.0 - w1
    return i0.to(dev), i1.to(dev), w0.to(dev), w1.to(dev)


def bilinear_up(src_nhwc, H, W, weight_round):
    """src (N,Hs,Ws,C) fp32 -> (N,H,W,C): sum of the four taps x weights; weight_round rounds the four PRODUCT weights (bf16 in
    upsample_add's bf16 path and in the head's gather, identity in the head's folded branches and in the fp32 engine)."""
    N, Hs, Ws, C = src_nhwc.shape
    dev = src_nhwc.device
    y0, y1, wy0, wy1 = lerp_tables(H, Hs, dev)
    x0, x1, wx0, wx1 = lerp_tables(W, Ws, dev)
    out = torch.zeros((N, H, W, C), dtype=torch.float32, device=dev)
    for yi, wy in ((y0, wy0), (y1, wy1)):
        rows = src_nhwc[:, yi]                                   # (N,H,Ws,C)
        for xi, wx in ((x0, wx0), (x1, wx1)):
            wgt = weight_round(wx[None, :] * wy[:, None])        # (H,W): lx.w * ly.w as the kernels form it
            out += rows[:, :, xi] * wgt[None, :, :, None]
    return out


def check(name, got, ref, rel, abs_, stats, kernel, flip_slack=None, flip_fraction=0.0, label=None):
    """|got - ref| <= rel |ref| + abs_ everywhere.  flip_slack (same shape, optional): where an INTERNAL bf16 rounding sits between
    two matrix products (the head's hidden vector) kernel and reference may round a few hidden values to different neighbours;
    then at most `flip_fraction` of the elements may exceed the tight tolerance, none may exceed tight + flip_slack, and the mean
    error stays far below either (a systematic error -- one pixel position of every tile -- fails all three).
    `label`: the schedule's own label of the launch that wrote `got` (plan_ops()['kernel']); the row counts its checks per label."""
    err = (got - ref).abs()
    tol = rel * ref.abs() + abs_
    bad = err > tol
    if flip_slack is not None:
        frac = float(bad.float().mean())
        assert frac <= flip_fraction, f'{kernel} / {name}: {frac:.2e} of the elements beyond the tight tolerance (allowed {flip_fraction:.0e})'
        assert float(err.mean()) <= 0.02 * float(tol.mean()), f'{kernel} / {name}: mean |err| {float(err.mean()):.3e}'
        tol = tol + flip_slack
        bad = err > tol
    worst = float((err / tol).max())
    row = stats.setdefault(kernel, dict(ops=0, elements=0, worst_err_over_tol=0.0, max_abs_err=0.0, worst_op=''))
    row['ops'] += 1
    row['elements'] += int(err.numel())
    row['max_abs_err'] = max(row['max_abs_err'], float(err.max()))
    if label is not None:
        row.setdefault('labels', {})[label] = row.get('labels', {}).get(label, 0) + 1
    if worst > row['worst_err_over_tol']:
        row['worst_err_over_tol'], row['worst_op'] = worst, name
    if bad.any():
        idx = [int(v) for v in torch.nonzero(bad)[0]]
        raise AssertionError(f'{kernel} / {name}: {int(bad.sum())} of {bad.numel()} elements beyond tolerance; first at {idx}: '
                             f'got {float(got[tuple(idx)])} want {float(ref[tuple(idx)])}; max |err| {float(err.max())}')


BF16_ULP = 2.0 ** -7          # largest ulp / |y| of a bf16 value
E4M3_ULP = 2.0 ** -3


def run_case(sncal, cuda, cfg, sd, x, dtype, fp8_layers=None, want_heat=True, net=None):
    """One forward with every op tapped; returns (ops, tensors dict (op idx, tensor id) -> torch tensor, net).  `net`: a loaded (fp8:
    calibrated) network to run instead of a fresh one (tests/test_handoff_gpu.py: the state a re-calibration left behind)."""
    global X3_T
    global X3_SLACK
    X3_T = torch.float16 if sncal._lib.lib().sncal_x3_name() == b'fp16x3' else torch.bfloat16
    X3_SLACK = 2e-6 if X3_T == torch.float16 else 3e-5
    if net is None:
        net = sncal.HRNetHeatmap(cfg, dtype=dtype, device=cuda)
        net.load_state_dict(sd)
        if dtype == 'fp8':
            net.calibrate_fp8(x)
    if dtype == 'fp8':
        net.set_fp8_layers(fp8_layers or 'all')
    net.set_profiling(1)                                    # labels: which kernel served which op
    net.forward(x, want_heat=want_heat, decode_size=(540, 960) if net.cfg.get('head', 'logsoftmax') == 'logsoftmax' else None)
    torch.cuda.synchronize()
    ops = net.plan_ops()
    net.last_profile = net.get_profile()                    # the rows of this ONE forward (set_profiling clears them)
    net.set_profiling(0)
    taps = {}
    for op in ops:
        if not op['active'] or op['type'] == 'decode':
            continue
        ids = [op['in'], op['res'], op['out'], op['base'], op['head_direct']] + op['src'] + op['head_src'] + op['head_fold']
        for t in ids:
            if t is None or t < 0:
                continue
            info = net.plan_tensor(t)
            cand = [t] + ([info['twin']] if info['twin'] >= 0 else [])
            for tid in cand:
                if net.plan_tensor(tid)['alive'] and (op['idx'], tid) not in taps:
                    taps[(op['idx'], tid)] = net.tap(op['idx'], tid)
    net.forward(x, want_heat=want_heat, decode_size=(540, 960) if net.cfg.get('head', 'logsoftmax') == 'logsoftmax' else None)
    torch.cuda.synchronize()
    net.clear_taps()
    return ops, taps, net


def verify_plan(sncal, cuda, cfg, sd, x, dtype, fp8_layers=None, tag='', net=None):
    ops, taps, net = run_case(sncal, cuda, cfg, sd, x, dtype, fp8_layers, net=net)
    W = Weights(net, sd, cuda)
    f32_engine = dtype in ('fp32', 'fp16x3')
    act_round = (lambda t: t) if f32_engine else bf16r
    rel_out = 1e-5 if f32_engine else BF16_ULP
    abs_out = 2e-4 if f32_engine else 1e-3
    stats = {}
    B = min(x.shape[0], net.plan_tensor(0)['sub_batch'])
    x = x[:B]
    by_idx = {op['idx']: op for op in ops}
    label = ''
    fused_second = set()
    # which kernel served which convolution, from the schedule's own labels (the first op of a launch carries the label, `launch` names
    # the launch of every op it covers): stats['_case']['served'], one entry per active conv op that was checked
    launch_label = {o['launch']: o['kernel'] for o in ops if o['active'] and o['kernel']}
    launch_size = {}
    for o in ops:
        if o['active'] and o['launch'] >= 0:
            launch_size[o['launch']] = launch_size.get(o['launch'], 0) + 1
    served = []

    def serve(o, forms):
        served.append(dict(op=o['idx'], name=o['name'], cin=o['cin'], cout=o['cout'], ksize=o['ksize'], stride=o['stride'], fp8=bool(o['fp8']),
                           kernel=launch_label.get(o['launch'], ''), launch=o['launch'], members=launch_size.get(o['launch'], 0), forms=forms))

    def T(op, tid):
        return taps[(op['idx'], tid)]

    for op in ops:
        if not op['active']:
            continue
        if op['kernel']:
            label = op['kernel']                      # grouped members / the second conv of a fused block carry no label of their own
        if op['type'] == 'input':
            got = T(op, op['out']).to(torch.float32)
            ref = torch.zeros_like(got)
            ref[..., :3] = act_round(nhwc(x))
            check('input layout', got, ref, 0.0, 0.0, stats, 'nchw_to_nhwc')
        elif op['type'] == 'conv':
            if op['idx'] in fused_second:
                continue
            w, shift = W.get(op)
            ti = net.plan_tensor(op['in'])
            if label == 'bblock48_fused' and op['kernel'] == 'bblock48_fused':
                nxt = by_idx[op['idx'] + 1]
                assert nxt['type'] == 'conv' and nxt['in'] == op['out'] and nxt['res'] == op['in'], 'fused block shape'
                fused_second.add(nxt['idx'])
                w2, shift2 = W.get(nxt)
                xin = nchw(taps[(nxt['idx'], op['in'])])                       # x as it stood when the fused launch was done
                mid = bf16r(torch.relu(conv_ref(xin, bf16r(w), 1) + shift[None, :, None, None]))
                ref = conv_ref(mid, bf16r(w2), 1) + shift2[None, :, None, None] + xin
                ref = torch.relu(ref)
                got = nchw(taps[(nxt['idx'], nxt['out'])])
                # the intermediate tile is rounded to bf16 between the two convolutions: where kernel and reference round a mid value to
                # different neighbours (their fp32 sums differ in the last bits) the output moves by ulp(mid) x |w2| ~ 4e-4 per flip
                check(op['name'] + ' + conv2', got, ref, rel_out, 4e-3, stats, 'bblock48_fused', label=launch_label.get(op['launch'], label))
                serve(op, ['lds']), serve(nxt, ['dense'])
                continue
            if label == 'bblockx3_fused' and op['kernel'] == 'bblockx3_fused':
                # fp16x3, fused 48-channel BasicBlock (bblockx3.hip): x (split twin) -> conv1 + shift, ReLU -> mid (split in LDS, never in
                # HBM) -> conv2 + shift + x, ReLU -> split twin and / or fp32.  Every product good to ~2^-16: 3e-5 of sum |x w| per
                # convolution, the first one's bound carried through |w2|
                nxt = by_idx[op['idx'] + 1]
                assert nxt['type'] == 'conv' and nxt['in'] == op['out'] and nxt['res'] == op['in'], 'fused block shape'
                fused_second.add(nxt['idx'])
                w2, shift2 = W.get(nxt)
                xin = _split_twin_value(taps[(nxt['idx'], ti['twin'])])
                mid = torch.relu(conv_ref(xin, w, 1) + shift[None, :, None, None])
                y = torch.relu(conv_ref(mid, w2, 1) + shift2[None, :, None, None] + xin)
                slack = X3_SLACK * conv_ref(mid.abs(), w2.abs(), 1) + conv_ref(X3_SLACK * conv_ref(xin.abs(), w.abs(), 1), w2.abs(), 1)
                to = net.plan_tensor(nxt['out'])
                name = f"{op['name']} + conv2 {to['H']}x{to['W']} 48->48->48"
                checked = False
                if to['alive'] and nxt['writes_out']:
                    got = nchw(taps[(nxt['idx'], nxt['out'])])[:, nxt['out_coff']:nxt['out_coff'] + 48]
                    check(name, got, y, rel_out, abs_out + slack, stats, 'bblockx3_fused')
                    checked = True
                if nxt['writes_twin']:
                    check(name + ' [split twin out]', _split_twin_value(taps[(nxt['idx'], to['twin'])]), y, 1e-5 + 2.0 ** -16, abs_out + slack, stats, 'bblockx3_fused split out')
                    checked = True
                assert checked, name
                serve(op, ['lds']), serve(nxt, ['dense'] * bool(to['alive'] and nxt['writes_out']) + ['twin'] * bool(nxt['writes_twin']))
                continue
            if label == 'bneck_tail_ds_x3' and op['kernel'] == 'bneck_tail_ds_x3':
                # fp16x3, layer1 block 0 (bneckx3.hip): this op is the downsample branch, the next one the conv3 that adds it; one launch
                # computes ReLU(W3 . h2 + shift3 + Wds . x0 + shift_ds), the 256-channel branch tensor is never written
                nxt = by_idx[op['idx'] + 1]
                assert nxt['type'] == 'conv' and nxt['res'] == op['out'] and nxt['relu'] and not op['relu'], 'fused tail shape'
                fused_second.add(nxt['idx'])
                w3, shift3 = W.get(nxt)
                x0 = nchw(T(op, op['in']))[:, :op['cin']]
                h2 = nchw(taps[(nxt['idx'], nxt['in'])])[:, :nxt['cin']]
                y = torch.relu(conv_ref(h2, w3, 1) + shift3[None, :, None, None] + conv_ref(x0, w, 1) + shift[None, :, None, None])
                slack = X3_SLACK * (conv_ref(h2.abs(), w3.abs(), 1) + conv_ref(x0.abs(), w.abs(), 1))
                to = net.plan_tensor(nxt['out'])
                got = nchw(taps[(nxt['idx'], nxt['out'])])
                check(f"{nxt['name']} + downsample {to['H']}x{to['W']} 64+64->256", got, y, rel_out, abs_out + slack, stats, 'bneck_tail_ds_x3', label=launch_label.get(op['launch'], label))
                serve(op, ['lds']), serve(nxt, ['dense'])
                continue
            if op['fp8']:
                tw = net.plan_tensor(ti['twin'])
                xin = e4m3_decode(T(op, ti['twin'])).permute(0, 3, 1, 2).contiguous()            # codes
                wmax = w.abs().amax(dim=(1, 2, 3))
                wscale = torch.where(wmax > 0, wmax / 448.0, torch.ones_like(wmax))
                wq = e4m3_round(w / wscale[:, None, None, None])
                oscale = (torch.tensor(tw['scale'], dtype=torch.float32, device=cuda) * wscale)  # fp32 product, as the host forms it
                y = conv_ref(xin, wq, 1) * oscale[None, :, None, None] + shift[None, :, None, None]
                # v_mfma_scale_f32_32x32x64_f8f6f4 does NOT accumulate in full fp32 (tools/dev/fp8_acc_probe.hip, measured): the 64
                # products of a K block are summed in groups of 8 whose members are aligned to the group's largest product and
                # TRUNCATED 2^-13 below it (a 2^8 product keeps 2^-5 neighbours exactly and drops 2^-6 ones entirely).  Each term can
                # lose up to 2^-13 of its group's maximum: <= 7 x 2^-14 of the sum of |x w| on average, one-sided.  Measured on these
                # layers: up to 1.5e-4 = 2^-12.7 of sum |x w|; allowed: 2^-11 of it (a wrong tap moves the sum by ~2^-6 of it)
                fp8_slack = 2.0 ** -11 * conv_ref(xin.abs(), wq.abs(), 1) * oscale[None, :, None, None]
            elif op.get('x3'):
                # fp16x3: fp32 operands split into bf16 hi + lo, hi.hi + hi.lo + lo.hi in fp32: every product is good to ~2^-16 of
                # itself, so the sum is good to a few 1e-5 of sum |x w| (measured below 1e-5); a wrong tap is 2^-6 of it
                raw = T(op, ti['twin'])                       # the operand the kernel reads: the split twin, hi + lo = x to 2^-17
                pr = raw.view(X3_T).reshape(raw.shape[0], raw.shape[1], raw.shape[2], raw.shape[3] // 16, 2, 16).to(torch.float32)
                xin = (pr[..., 0, :] + pr[..., 1, :]).reshape(raw.shape).permute(0, 3, 1, 2).contiguous()
                y = conv_ref(xin, w, op['stride']) + shift[None, :, None, None]
                fp8_slack = X3_SLACK * conv_ref(xin.abs(), w.abs(), op['stride'])
            else:
                xin = nchw(T(op, op['in']))[:, :op['cin']]
                y = conv_ref(xin, act_round(w), op['stride']) + shift[None, :, None, None]
                # fp16x3 engine, generic kernel (x3_t): fp32 operands split in registers, same arithmetic and the same bound as above
                fp8_slack = X3_SLACK * conv_ref(xin.abs(), w.abs(), op['stride']) if op.get('x3g') else 0.0
            if op['res'] >= 0 and op.get('res_twin'):
                # fp16x3, inside a BasicBlock chain: the block input lives only as the split twin its first convolution read
                raw = T(op, net.plan_tensor(op['res'])['twin'])
                pr = raw.view(X3_T).reshape(raw.shape[0], raw.shape[1], raw.shape[2], raw.shape[3] // 16, 2, 16).to(torch.float32)
                y = y + (pr[..., 0, :] + pr[..., 1, :]).reshape(raw.shape).permute(0, 3, 1, 2)
            elif op['res'] >= 0:
                y = y + nchw(T(op, op['res']))[:, op['out_coff']:op['out_coff'] + op['cout']]
            if op['relu']:
                y = torch.relu(y)
            to = net.plan_tensor(op['out'])
            kern = 'conv_tt<fp8,k3,s1,8x32x96>' if op['fp8'] else ('conv_tt<fp16x3,k3,s1,12x32x64>' if op['cout'] % 96 else 'conv_tt<fp16x3,k3,s1,8x32x96>') if op.get('x3') else label
            name = f"{op['name']} {to['H']}x{to['W']} {op['cin']}->{op['cout']}" + ('+res' if op['res'] >= 0 else '')
            real = launch_label.get(op['launch'], label)                # the schedule's label of the launch that really served this op
            forms = []
            checked = False
            gen_twin = bool(op.get('x3g')) and op['writes_twin']
            if gen_twin:
                check(name + ' [split twin out]', _split_twin_value(T(op, to['twin'])), y, 1e-5 + 2.0 ** -16, abs_out + fp8_slack, stats, kern + ' split out', label=real)
                checked = True
                forms.append('twin')
            if to['alive'] and op['writes_out']:
                got = nchw(T(op, op['out']))[:, op['out_coff']:op['out_coff'] + op['cout']]
                if op['out_f32']:
                    check(name, got, y, 1e-5 if f32_engine else 2.0 ** -9, abs_out, stats, kern, label=real)     # fp32 logits of bf16 operands
                else:
                    check(name, got, y, rel_out, abs_out + fp8_slack, stats, kern, label=real)
                checked = True
                forms.append('dense')
            if op.get('x3') and op['writes_twin']:
                # split twin written by the epilogue: [16 hi | 16 lo] bf16 per 16-channel group; hi + lo reproduces y to 2^-17
                raw = T(op, to['twin'])                                                  # fp32-typed storage, (N,H,W,C)
                pr = raw.view(X3_T).reshape(raw.shape[0], raw.shape[1], raw.shape[2], raw.shape[3] // 16, 2, 16).to(torch.float32)
                got_t = (pr[..., 0, :] + pr[..., 1, :]).reshape(raw.shape).permute(0, 3, 1, 2)
                check(name + ' [split twin out]', got_t, y, 1e-5 + 2.0 ** -16, abs_out + fp8_slack, stats, kern + ' split out', label=real)
                checked = True
                forms.append('twin')
            if op['fp8'] and op['writes_twin']:
                tw_o = net.plan_tensor(to['twin'])
                got8 = e4m3_decode(T(op, to['twin'])).permute(0, 3, 1, 2) * tw_o['scale']
                ref8 = e4m3_round(bf16r(y) / tw_o['scale']) * tw_o['scale']
                check(name + ' [e4m3 out]', got8, ref8, E4M3_ULP, tw_o['scale'] * 2.0 ** -9 + 1e-3 + fp8_slack, stats, kern + ' e4m3 out', label=real)
                checked = True
                forms.append('e4m3')
            assert checked, name
            serve(op, forms)
        elif op['type'] == 'upsample_add':
            to = net.plan_tensor(op['out'])
            wr = (lambda t: t) if f32_engine else bf16r
            acc = None
            C0 = None
            for s in op['src']:
                src = T(op, s).to(torch.float32)
                C0 = src.shape[-1]
                up = bilinear_up(src, to['H'], to['W'], wr)
                acc = up if acc is None else acc + up
            if op['base'] >= 0:
                acc = acc + T(op, op['base']).to(torch.float32)
            if op['relu']:
                acc = torch.relu(acc)
            nm = f"fuse sum -> {to['H']}x{to['W']}x{C0} ({len(op['src'])} sources)"
            tw = op['writes_twin']
            if tw:          # fp16x3: the sum's split twin for the two-team convolution that reads it; the fp32 form only if somebody reads that
                check(nm + ' [split twin out]', _split_twin_value(T(op, to['twin'])).permute(0, 2, 3, 1), acc, 1e-5 + 2.0 ** -16, abs_out, stats, 'upsample_add split out')
            if op['writes_out']:
                got = T(op, op['out']).to(torch.float32)[..., op['out_coff']:op['out_coff'] + C0]
                check(nm, got, acc, rel_out, abs_out, stats, 'upsample_add')
        elif op['type'] == 'head':
            head_reference(net, op, T, W, by_idx, stats, cuda, exact=f32_engine)
        elif op['type'] == 'softmax':
            logits = T(op, op['in'])                                       # (N,H,W,Cpad) fp32
            C = net.num_classes
            to = net.plan_tensor(op['out'])
            got = T(op, op['out']).reshape(-1).view(logits.shape[0], C, to['H'], to['W'])     # the heat tensor is NCHW
            lg = logits[..., :C].permute(0, 3, 1, 2)
            ref = torch.softmax(lg, dim=1) if net.cfg.get('head') == 'softmax' else torch.log_softmax(lg, dim=1)
            check('softmax head', got, ref, 1e-5, 1e-5, stats, 'softmax_nchw')
    pairs, skipped = producer_reader_identity(net, ops, taps)
    twins = twin_value_identity(net, ops, taps, dtype, stats, skipped)
    # no convolution went unchecked: every active conv op has exactly one entry in `served`, with at least one output form compared
    conv_active = [o['idx'] for o in ops if o['active'] and o['type'] == 'conv']
    assert sorted(e['op'] for e in served) == conv_active, (sorted(set(conv_active) - {e['op'] for e in served}), len(served), len(conv_active))
    assert all(e['forms'] and e['kernel'] for e in served), [e for e in served if not (e['forms'] and e['kernel'])][:3]
    stats['_case'] = dict(tag=tag, dtype=dtype, fp8_layers=fp8_layers, frames=int(B), input=list(x.shape[2:]),
                          reader_pairs=pairs, lds_intermediates=len(skipped), **twins, conv_ops_active=len(conv_active), conv_ops_checked=len(served),
                          served=served, profile_launches={p['kernel']: p['launches'] for p in getattr(net, 'last_profile', [])})
    return stats


# ---- between the launches: what a producer wrote is what every later reader found --------------------------------------------
FUSED_PAIR_KERNELS = ('bblock48_fused', 'bblockx3_fused', 'bneck_tail_ds_x3')     # their first op's output stays in LDS
X3_ENGINES = ('fp16x3', 'bf16x3', 'x3')


def _real_reads(net, o):
    """Tensor ids the launch of op `o` really reads for it: the twin in place of `in` for the e4m3 / split two-team convolutions (and
    `in` itself beside it when the schedule puts a helper in front of the launch to make the twin: prep_in), the twin in place of `res`
    for res_twin."""
    r = []
    if o['in'] >= 0:
        if o['type'] == 'conv' and (o['fp8'] or o.get('x3')):
            r.append(net.plan_tensor(o['in'])['twin'])
            if o['prep_in']:
                r.append(o['in'])
        else:
            r.append(o['in'])
    if o['res'] >= 0:
        r.append(net.plan_tensor(o['res'])['twin'] if o.get('res_twin') else o['res'])
    r += [o['base'], o['head_direct']] + o['src'] + o['head_src'] + o['head_fold']
    return [t for t in r if t is not None and t >= 0]


def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def producer_reader_identity(net, ops, taps):
    """The per-launch checks above recompute a launch from the operands it READ; a launch in between that clobbered a live tensor would
    hand the reader clobbered operands and pass.  So: for every allocated tensor and twin, the tap taken at its producing op equals, byte
    for byte, the tap taken at every later op that really reads it (last reader included); concat tensors per producer slice, from that
    producer's tap on.  Tensors no launch writes -- the intermediate of a fused pair, which stays in LDS -- are skipped, and the skipped
    set must be exactly the intermediates of the launches labelled as fused pairs.  Returns (pairs compared, skipped tensor ids)."""
    act = [o for o in ops if o['active'] and o['type'] != 'decode']
    producers = {}
    for o in act:
        if o['out'] is not None and o['out'] >= 0:
            producers.setdefault(o['out'], []).append(o)
    twin_of = {}
    for t in producers:
        tw = net.plan_tensor(t)['twin']
        if tw >= 0 and net.plan_tensor(tw)['alive']:
            twin_of[tw] = t
    readers = {}
    for o in act:
        for t in _real_reads(net, o):
            assert net.plan_tensor(t)['alive'], (o['idx'], t)
            readers.setdefault(t, []).append(o)
    for t in readers:
        assert t in producers or t in twin_of, f'tensor {t} is read and nobody writes it'
    # tensors that stay in LDS: produced and read inside ONE launch and nowhere else -- by the schedule, and by the labels
    by_idx = {o['idx']: o for o in ops}
    skipped = set()
    for t, rs in readers.items():
        p = producers[twin_of.get(t, t)][0]
        if p['launch'] >= 0 and all(r['launch'] == p['launch'] for r in rs):
            skipped.add(t)
    expected = set()
    for o in act:
        if o['kernel'] in FUSED_PAIR_KERNELS:
            nxt = by_idx[o['idx'] + 1]
            assert nxt['launch'] == o['launch'], (o['idx'], o['kernel'])
            expected |= {t for t in _real_reads(net, nxt) if twin_of.get(t, t) == o['out']}
    assert skipped == expected, f'tensors without a writer {sorted(skipped)} != intermediates of the fused pairs {sorted(expected)}'
    pairs = 0
    for t, rs in readers.items():
        if t in skipped:
            continue
        base = twin_of.get(t, t)
        in_front = t in twin_of and not any(p['writes_twin'] for p in producers[base])
        # (a twin its producer does not write is made in front of each reading launch, from the tensor -- itself compared as `base`)
        assert not in_front or rs[0]['prep_in'], f"twin {t} of tensor {base}: no producer writes it and op {rs[0]['idx']} reads it with no helper in front"
        writers = [rs[0]] if in_front else producers[base]
        for p in writers:
            lo, hi = 0, taps[(p['idx'], t)].shape[-1]
            if not in_front and (len(writers) > 1 or p['out_coff']):       # a channel slice of a concat tensor
                width = p['cout'] if p['type'] == 'conv' else net.plan_tensor(p['src'][0])['C']
                lo, hi = p['out_coff'], p['out_coff'] + width
            want = _bits(taps[(p['idx'], t)])[..., lo:hi]
            for r in rs:
                if r['idx'] <= p['idx']:
                    continue
                got = _bits(taps[(r['idx'], t)])[..., lo:hi]
                if not torch.equal(got, want):
                    n_bad = int((got != want).sum())
                    raise AssertionError(f"tensor {t}{' (twin of %d)' % base if t != base else ''} channels {lo}:{hi}: what op {p['idx']} "
                                         f"({p['name'] or p['type']}) wrote is not what op {r['idx']} ({r['name'] or r['type']}) read: "
                                         f"{n_bad} of {want.numel()} elements differ")
                pairs += 1
    assert pairs >= len(act), (pairs, len(act))         # every op reads something
    return pairs, skipped


# ---- a twin is the conversion of the dense tensor it stands for, bit for bit ------------------------------------------------
TWIN_ROWS = {('fp8', 'front'): 'quantize_fp8 in front', ('x3', 'front'): 'split_f32 in front',
             ('fp8', 'both'): 'e4m3 twin = q(dense)', ('x3', 'both'): 'split twin = split(dense)'}
QUANTIZE_GRID_ELEMENTS = 2048 * 256 * 8          # quant.hip: elements one trip of quantize_fp8_kernel's capped grid covers; a larger tensor
                                                 # takes the grid-stride loop round a second time (split_f32_kernel: 4096 * 256 * 8)


def twin_plan(net, ops, skipped):
    """From the plan alone (no taps): [(kind 'fp8' | 'x3', where 'front' | 'both', op, tensor id, twin id)].
    'front': the launch of `op` reads a twin its producer did not write, so quantize_fp8_kernel / split_f32_kernel makes it from the
    dense tensor in front of that launch (the op's prep_in).  'both': `op` writes its output AND the output's twin (its writes_out and
    writes_twin: the twin when a reduced-precision convolution reads it, the dense form when anybody else does).  The intermediates of
    the fused pairs (`skipped`) live in LDS and have neither form."""
    act = [o for o in ops if o['active'] and o['type'] != 'decode']
    producers = {}
    for o in act:
        if o['out'] is not None and o['out'] >= 0:
            producers.setdefault(o['out'], []).append(o)
    plan = []
    for o in act:
        if o['type'] == 'conv' and (o['fp8'] or o.get('x3')) and o['in'] >= 0:
            tw = net.plan_tensor(o['in'])['twin']
            if tw in skipped or o['in'] in skipped:
                continue
            assert tw >= 0 and net.plan_tensor(tw)['alive'], (o['idx'], o['in'], tw)
            if o['prep_in']:
                assert o['prep_in'] == (1 if o['fp8'] else 2), (o['idx'], o['prep_in'])
                plan.append(('fp8' if o['fp8'] else 'x3', 'front', o, o['in'], tw))
    for t, ps in producers.items():
        to = net.plan_tensor(t)
        tw = to['twin']
        if tw < 0 or not net.plan_tensor(tw)['alive'] or t in skipped or tw in skipped or len(ps) != 1:
            continue
        p = ps[0]
        if p['writes_twin'] and to['alive'] and p['writes_out']:
            plan.append(('fp8' if p['type'] == 'conv' and p['fp8'] else 'x3', 'both', p, t, tw))
    return plan


def twin_value_identity(net, ops, taps, dtype, stats, skipped=()):
    """producer_reader_identity shows that a twin did not change between its writer and its readers, and the per-launch checks recompute a
    launch from the twin it read: a helper or an epilogue that makes a self-consistent WRONG twin passes both.  So every twin is held to
    the dense tensor tapped at the same op, with no tolerance (tests/handoff_ref.py, pinned on the CPU by tests/test_handoff_host.py):

        split twin   codes == split16(dense fp32): xc = clamp(x, +-65504) (fp16 build), hi = rne16(xc), lo = rne16(xc - hi), [16 hi | 16 lo]
        e4m3 twin    decode(codes) == e4m3_rne(clamp(float(dense bf16) * (1.0f / scale), +-448)), as floats (+0 == -0)

    for the twins the helpers of quant.hip make in front of a launch, and for the twins an epilogue writes beside the dense output it also
    writes: conv_tt's x3 and fp8 epilogues, bblockx3, the generic convolution and upsample_add with a twin output all convert the very
    value they store (the fp8 epilogue the ROUNDED bf16 value), and x3.hpp's fused v_fma_mix spelling gives the bits of the plain one.
    The seams of layer1 (bneckx3.hip) write no twin at all (hrnet_schedule.cpp fuses_bneck_seam requires that nobody is owed one), and a
    producer that writes ONLY the twin (inside a BasicBlock chain) leaves no dense form to compare with: its twin stays with the per-launch
    tolerance.  How many pairs there are comes from the plan (twin_plan); exactly that many are compared.  Rows of `stats`, for the engine
    that has twins: the four of TWIN_ROWS (ops = pairs, sites = pairs per kernel label).  Returns the counts for stats['_case'], with the
    largest tensor a helper converted in front of a launch (its capped grid-stride loop, QUANTIZE_GRID_ELEMENTS)."""
    import handoff_ref as hr
    plan = twin_plan(net, ops, skipped)
    largest = {'fp8': 0, 'x3': 0}
    rows = {}
    labels = {o['launch']: o['kernel'] for o in ops if o['active'] and o['kernel']}      # (grouped / fused members carry no label of their own)
    for kind, where, op, t, tw in plan:
        assert (op['idx'], t) in taps and (op['idx'], tw) in taps, f"op {op['idx']}: tensor {t} / twin {tw} not tapped"
        dense, twin = taps[(op['idx'], t)], taps[(op['idx'], tw)]
        what = f"{TWIN_ROWS[(kind, where)]}: op {op['idx']} ({op['name'] or op['type']}), tensor {t} {tuple(dense.shape)}, twin {tw}"
        if kind == 'x3':
            assert dense.dtype == torch.float32 and twin.shape == dense.shape, what
            got, want = hr.split_codes_of_twin(twin), hr.split16(dense, X3_T)
            show = lambda v: f'0x{int(v) & 0xffff:04x}'
        else:
            scale = net.plan_tensor(tw)['scale']
            assert dense.dtype == torch.bfloat16 and twin.dtype == torch.uint8 and twin.shape == dense.shape and scale > 0, what
            got, want = hr.e4m3_values(twin), hr.e4m3_values(hr.e4m3_codes(dense, scale))
            what += f', scale {scale!r}'
            show = float
        bad = got != want
        if bad.any():
            idx = tuple(int(v) for v in torch.nonzero(bad)[0])
            src = idx if kind == 'fp8' else idx[:3] + (idx[3] // 32 * 16 + idx[3] % 16,)
            raise AssertionError(f'{what}: {int(bad.sum())} of {bad.numel()} twin elements are not the conversion of the dense tensor; first at '
                                 f'{list(idx)} ({"hi" if kind == "x3" and idx[3] % 32 < 16 else "lo" if kind == "x3" else "code"}): twin holds '
                                 f'{show(got[idx])}, dense {float(dense[src])!r} converts to {show(want[idx])}')
        row = rows.setdefault((kind, where), dict(ops=0, elements=0, worst_err_over_tol=0.0, max_abs_err=0.0, worst_op=''))
        row['ops'] += 1
        row['elements'] += int(dense.numel())
        site = labels.get(op['launch'], op['type'])                 # which kernel's launch read (front) / wrote (both) the pair
        row.setdefault('sites', {})[site] = row.get('sites', {}).get(site, 0) + 1
        if where == 'front':
            largest[kind] = max(largest[kind], int(dense.numel()))
    expected = {}
    for kind, where, *_ in plan:
        expected[(kind, where)] = expected.get((kind, where), 0) + 1
    engine = 'fp8' if dtype == 'fp8' else 'x3' if dtype in X3_ENGINES else None
    for key, name in TWIN_ROWS.items():
        n = rows.get(key, {'ops': 0})['ops']
        assert n == expected.get(key, 0), (name, n, expected.get(key, 0))
        assert key[0] == engine or n == 0, (name, dtype, n)
        if key[0] == engine:
            stats[name] = rows.get(key, dict(ops=0, elements=0, worst_err_over_tol=0.0, max_abs_err=0.0, worst_op=''))
    return dict(twin_pairs_expected=len(plan), twin_pairs_compared=sum(r['ops'] for r in rows.values()),
                largest_quantize_in_front=largest['fp8'], largest_split_in_front=largest['x3'])


def _split_twin_value(raw):
    """(N,H,W,C) fp32-typed storage of a split twin -> (N,C,H,W) fp32: hi + lo."""
    pr = raw.view(X3_T).reshape(raw.shape[0], raw.shape[1], raw.shape[2], raw.shape[3] // 16, 2, 16).to(torch.float32)
    return (pr[..., 0, :] + pr[..., 1, :]).reshape(raw.shape).permute(0, 3, 1, 2)


def head_reference(net, op, T, W, by_idx, stats, dev, exact=False):
    """head32.hip / head.hip on their own operands: hidden = relu(b0 + W0[:, :K1] . [direct | up(narrow branches)] + sum_s up(t_s)),
    logits = W1 . bf16(hidden) + b1, with the roundings the kernel applies (bf16 blends of the folded branches, bf16 gather
    weights, bf16 hidden vector)."""
    to = net.plan_tensor(op['out'])
    H, Wd = to['H'], to['W']
    rnd = (lambda t: t) if exact else bf16r          # fp16x3 engine (headx3.hip): fp32 operands, every product good to ~2^-16
    direct = T(op, op['head_direct']).to(torch.float32)                    # (N,H,W,Cd)
    parts = [direct]
    for f in op['head_fold']:
        parts.append(rnd(bilinear_up(T(op, f).to(torch.float32), H, Wd, lambda t: t)))
    kin = torch.cat(parts, dim=-1)                                          # (N,H,W,K1)
    K1 = kin.shape[-1]
    units = W.units
    _, bn0, cin0, cout0, _, _, hb0 = units['model.last_layer.0']
    w0, sc0, sh0 = folded(W.sd, 'model.last_layer.0', bn0, hb0)
    w0s = rnd((w0 * sc0[:, None, None, None])[:, :K1, 0, 0].to(dev))      # (784,K1)
    hid = kin.reshape(-1, K1) @ w0s.t() + sh0.to(dev)[None]
    hid = hid.reshape(kin.shape[0], H, Wd, cout0)
    for s in op['head_src']:
        t = T(op, s).to(torch.float32)[..., :cout0]
        hid = hid + bilinear_up(t, H, Wd, rnd)
    hid = rnd(torch.relu(hid))
    _, _, cin1, cout1, _, _, hb1 = units['model.last_layer.3']
    w1, sc1, sh1 = folded(W.sd, 'model.last_layer.3', '', hb1)
    w1s = rnd(w1[:, :, 0, 0].to(dev))
    ref = hid.reshape(-1, cout0) @ w1s.t() + sh1.to(dev)[None]
    ref = ref.reshape(kin.shape[0], H, Wd, cout1)
    got = T(op, op['out'])[..., :cout1]
    if exact:
        check(f'head -> logits {H}x{Wd} (split-fp16)', got, ref, 1e-4, 5e-4, stats, 'headx3_fused')
        return
    # the hidden vector is rounded to bf16 BEFORE the 784-term second product: a hidden value whose fp32 sums differ in the last bits
    # between kernel and reference rounds to the other neighbour (one bf16 ulp of that hidden unit x |w1|).  Per element: up to eight
    # flips of the pixel's largest hidden value; measured 2e-5 .. 2e-3 of the elements leave the tight tolerance that way
    hmax = hid.amax(dim=-1, keepdim=True)                                   # (N,H,W,1)
    ulp = torch.exp2(torch.floor(torch.log2(hmax.clamp(min=2.0 ** -20))) - 7.0)
    flip = 8.0 * ulp * w1s.abs().amax(dim=1)[None, None, None, :]
    check(f'head -> logits {H}x{Wd}', got, ref, 2.0 ** -9, 4e-3, stats, 'head_fused', flip_slack=flip, flip_fraction=5e-3)


def _weights(cfg):
    import bench
    return bench.seeded_weights(cfg, seed=1)


def _report(stats, name):
    print('KERNEL-PARITY', json.dumps(stats))
    try:
        os.makedirs('gpurun_out', exist_ok=True)
        with open(os.path.join('gpurun_out', f'kernel_parity_{name}.json'), 'w') as f:
            json.dump(stats, f, indent=1)
    except OSError:
        pass


def _twin_rows(stats, *rows):
    """The twin checks of this case were not vacuous: as many pairs compared as the plan holds, each named row at least once."""
    c = stats['_case']
    assert c['twin_pairs_compared'] == c['twin_pairs_expected'] > 0, c
    for r in rows:
        assert r in stats and stats[r]['ops'] >= 1, (r, c, {k: stats[k]['ops'] for k in TWIN_ROWS.values() if k in stats})


FP8_TWIN_ROWS = ('quantize_fp8 in front', 'e4m3 twin = q(dense)')
# The split engine's producers -- the two-team and generic convolutions, bblockx3, the fuse sums -- write every twin a stock network
# (W18 / W32 / W48, line network; 140p .. 1080p) reads, so NO launch of such a plan has split_f32_kernel in front (no op reports prep_in == 2:
# tests/test_workspace_gpu.py _audit_forms asserts it over every audited layout): the row is reported, with compared == expected == 0, and
# nothing is asserted about a path the engine does not take.
X3_TWIN_ROWS = ('split twin = split(dense)',)


def _frames(B, H, W, seed, dev):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((B, 3, H, W), generator=g, dtype=torch.float32).to(dev)


def test_every_launch_of_the_bf16_engine_w48_540p(sncal, cuda):
    """The benchmarked engine at the metric's size, 3 frames: branch maps 135x240 / 68x120 / 34x60 / 17x30 (partial 32-pixel tiles on
    every branch, two stacked-frame boundaries inside the tiles)."""
    sd = _weights('hrnet_w48')
    stats = verify_plan(sncal, cuda, 'hrnet_w48', sd, _frames(3, 540, 960, 11, cuda), 'bf16', tag='w48 540p')
    _report(stats, 'bf16_w48_540p')
    for k in ('conv_tt<bf16,k3,s1,8x32x96>', 'bblock48_fused', 'head_fused', 'upsample_add'):
        assert k in stats and stats[k]['ops'] > 0, (k, list(stats))
    assert any(k.startswith('conv<bf16,k3,s2') for k in stats) and any(k.startswith('conv<bf16,k1,s1') for k in stats)
    assert stats['conv_tt<bf16,k3,s1,8x32x96>']['ops'] == 144 and stats['bblock48_fused']['ops'] == 32


def test_every_launch_of_the_bf16_engine_w48_1080p(sncal, cuda):
    """C5's shapes (270x480 / 135x240 / 68x120 / 34x60 branches, 540x960 head), 2 frames."""
    sd = _weights('hrnet_w48')
    stats = verify_plan(sncal, cuda, 'hrnet_w48', sd, _frames(2, 1080, 1920, 12, cuda), 'bf16', tag='w48 1080p')
    _report(stats, 'bf16_w48_1080p')
    assert stats['conv_tt<bf16,k3,s1,8x32x96>']['ops'] == 144 and stats['bblock48_fused']['ops'] == 32


def test_every_launch_of_the_bf16_engine_odd_sizes(sncal, cuda):
    """270x500 input: 68x125 / 34x63 / 17x32 / 9x16 maps -- widths that are not multiples of the tiles, a 9-row branch (stacked
    frames interleave inside one 8-row tile), and the stem-interpolation head path."""
    sd = _weights('hrnet_w48')
    stats = verify_plan(sncal, cuda, 'hrnet_w48', sd, _frames(5, 270, 500, 13, cuda), 'bf16', tag='w48 270x500')
    _report(stats, 'bf16_w48_270x500')
    assert stats['conv_tt<bf16,k3,s1,8x32x96>']['ops'] == 144


@pytest.mark.parametrize('dtype', ['bf16', 'fp16x3'])
def test_every_launch_with_partial_head_tiles_in_both_directions(sncal, cuda, dtype):
    """2 frames of 140x240: a 70x120 head on the fused 32-wide kernels (head32.hip / headx3.hip, tiles of 4 rows x 32 columns) whose
    last row tile holds 2 of 4 rows AND whose last column tile holds 24 of 32 columns -- the `valid` / column masks of the shared
    epilogue and logits store (head_frame.hpp); the 540p and 1080p heads have full column tiles, 270x500 takes the unfused head.
    The profile labels the bf16 head by engine, not by kernel: that head32.hip (and not head.hip's 16-wide kernel) serves this shape is
    what tests/test_hrnet_gpu.py::test_fused_logsoftmax_decode_is_bit_identical asserts at 140x240 (only head32 fuses the decode)."""
    sd = _weights('hrnet_w48')
    stats = verify_plan(sncal, cuda, 'hrnet_w48', sd, _frames(2, 140, 240, 24, cuda), dtype, tag='w48 140x240 ' + dtype)
    _report(stats, dtype + '_w48_140x240')
    assert ('head_fused' if dtype == 'bf16' else 'headx3_fused') in stats, list(stats)      # not some other head path
    if dtype != 'bf16':
        _twin_rows(stats, *X3_TWIN_ROWS)


@pytest.mark.parametrize('layers', ['all', 'stage4,c192,c384'])
def test_every_launch_of_the_fp8_engine_w48_540p(sncal, cuda, layers):
    """C5 arithmetic: the e4m3 convolutions against torch fp32 on the e4m3 codes they read (per-tensor input scale x per-channel
    weight scale folded into the reference), their bf16 outputs and their e4m3 twin outputs; everything else as the bf16 engine."""
    sd = _weights('hrnet_w48')
    stats = verify_plan(sncal, cuda, 'hrnet_w48', sd, _frames(3, 540, 960, 14, cuda), 'fp8', fp8_layers=layers, tag='w48 540p fp8 ' + layers)
    _report(stats, 'fp8_w48_540p_' + layers.replace(',', '_'))
    k = 'conv_tt<fp8,k3,s1,8x32x96>'
    assert k in stats and k + ' e4m3 out' in stats
    n8 = stats[k]['ops'] + 0
    assert (stats[k + ' e4m3 out']['ops'] > 0) and (n8 > 0)
    if layers == 'all':
        assert stats[k]['ops'] + stats[k + ' e4m3 out']['ops'] >= 144          # every one of the 144 wide convolutions checked on at least one output
        assert stats[k + ' e4m3 out']['ops'] >= 120                            # all but the last convolution of each chain hand an e4m3 twin on
    _twin_rows(stats, *FP8_TWIN_ROWS)


def test_every_launch_of_the_fp8_engine_w48_1080p(sncal, cuda):
    sd = _weights('hrnet_w48')
    stats = verify_plan(sncal, cuda, 'hrnet_w48', sd, _frames(2, 1080, 1920, 15, cuda), 'fp8', fp8_layers='all', tag='w48 1080p fp8')
    _report(stats, 'fp8_w48_1080p')
    assert 'conv_tt<fp8,k3,s1,8x32x96>' in stats
    _twin_rows(stats, *FP8_TWIN_ROWS)
    # two frames of the 135x240x96 branch are 6.2 M elements: quantize_fp8_kernel's capped grid goes round its loop a second time
    assert stats['_case']['largest_quantize_in_front'] > QUANTIZE_GRID_ELEMENTS, stats['_case']


def test_every_launch_of_the_line_network_bf16(sncal, cuda):
    """L1: the line network (no upscale, 720-channel head, Softmax) -- the head's other configuration."""
    sd = _weights('line_hrnet_w48')
    stats = verify_plan(sncal, cuda, 'line_hrnet_w48', sd, _frames(3, 540, 960, 16, cuda), 'bf16', tag='line w48 540p')
    _report(stats, 'bf16_line_w48_540p')
    assert 'head_fused' in stats and 'softmax_nchw' in stats


def test_every_launch_of_the_fp32_engine_w18(sncal, cuda):
    """The exact engine's kernels one by one (fp32 MFMA generic conv, fp32 upsample / concat, reference-formulation head)."""
    from oracle import hrnet_ref as hr
    cfg = hr.load_config('hrnet_w18')
    sd = hr.seeded_state_dict(cfg, 3, 4.0)
    stats = verify_plan(sncal, cuda, 'hrnet_w18', sd, _frames(3, 135, 240, 17, cuda), 'fp32', tag='w18 135x240 fp32')
    _report(stats, 'fp32_w18_135x240')
    assert any(k.startswith('conv<f32') for k in stats)


@pytest.mark.parametrize('small_items', ['2', '0'])
def test_every_launch_of_the_fp16x3_engine_w48_540p(sncal, cuda, monkeypatch, small_items):
    """The fp32-class engine: fp32 tensors everywhere, the 3x3 stride-1 convolutions of stages 2-4 (wide branches and the 48-channel
    branch as fused BasicBlocks, bblockx3.hip) in split-fp16 arithmetic -- each against torch fp32 on the
    split twin it reads (hi + lo; written by the producing convolution's epilogue or by split_f32_kernel), its fp32 output and the
    split twin it hands on.  Twice: three frames are a SMALL launch and take the two-team kernel's 96 x 4 x 32 tile by default
    (SNCAL_TT_SMALL_ITEMS = 2 items per team, hrnet_schedule.cpp tt_cfg); 0 forces the 96 x 8 x 32 tile of the large batches."""
    monkeypatch.setenv('SNCAL_TT_SMALL_ITEMS', small_items)
    sd = _weights('hrnet_w48')
    stats = verify_plan(sncal, cuda, 'hrnet_w48', sd, _frames(3, 540, 960, 18, cuda), 'fp16x3', tag='w48 540p fp16x3 small tile ' + small_items)
    _report(stats, 'fp16x3_w48_540p' + ('' if small_items == '2' else '_tile8'))
    k, kb = 'conv_tt<fp16x3,k3,s1,8x32x96>', 'bblockx3_fused'   # 144 wide convolutions + 32 fused 48-channel blocks, each checked on its fp32 output, its twin, or both
    n = lambda key: stats.get(key, {'ops': 0})['ops']
    assert n(k) >= 12 and n(k + ' split out') >= 120                                         # (fp32 outputs: module ends only)
    assert n(k) + n(k + ' split out') >= 144 and n(kb) + n(kb + ' split out') >= 32 and n(kb) >= 8 and n(kb + ' split out') >= 24
    # layer1 (bneckx3.hip): block 0's conv3 with its downsample branch inside, and the seams conv3 + next conv1 of blocks 1 | 2 and 2 | 3
    # (two checks each: the 256-channel block output and the next block's 64-channel conv1 output)
    assert n('bneck_tail_ds_x3') == 1 and n('bneck_seam_x3') == 4, {k: v.get('ops') for k, v in stats.items()}
    _twin_rows(stats, *X3_TWIN_ROWS)


def test_every_launch_of_the_fp16x3_engine_w32_270p(sncal, cuda):
    """BASELINE config C2's shapes (HRNet-W32, 480x270): branch widths 32 / 64 / 128 / 256 all run as 64-channel blocks of the
    64 x 12 x 32 tile (the 32-channel branch half padded), maps 68x120 / 34x60 / 17x30 / 9x15 (a 9-row branch inside 12-row tiles)."""
    sd = _weights('hrnet_w32')
    stats = verify_plan(sncal, cuda, 'hrnet_w32', sd, _frames(5, 270, 480, 19, cuda), 'fp16x3', tag='w32 270p fp16x3')
    _report(stats, 'fp16x3_w32_270p')
    k48 = 'conv_tt<fp16x3,k3,s1,12x32x64>'
    n = lambda key: stats.get(key, {'ops': 0})['ops']
    assert n(k48) + n(k48 + ' split out') >= 200, {k: v['ops'] for k, v in stats.items()}
    assert any(k.startswith('conv<fp16x3,k3,s2') for k in stats) and any(k.startswith('conv<fp16x3,k1,s1') for k in stats)
    _twin_rows(stats, *X3_TWIN_ROWS)


def test_every_launch_of_the_fp16x3_engine_w48_1080p_and_odd_sizes(sncal, cuda):
    """C5's shapes (2 frames of 1920x1080) and a 270x500 input (68x125 / 34x63 / 17x32 / 9x16 maps, stem-interpolation head path)."""
    sd = _weights('hrnet_w48')
    stats = verify_plan(sncal, cuda, 'hrnet_w48', sd, _frames(2, 1080, 1920, 20, cuda), 'fp16x3', tag='w48 1080p fp16x3')
    _report(stats, 'fp16x3_w48_1080p')
    assert 'conv_tt<fp16x3,k3,s1,8x32x96> split out' in stats and stats['bblockx3_fused split out']['ops'] >= 24 and stats['bblockx3_fused']['ops'] >= 8
    _twin_rows(stats, *X3_TWIN_ROWS)
    stats = verify_plan(sncal, cuda, 'hrnet_w48', sd, _frames(5, 270, 500, 21, cuda), 'fp16x3', tag='w48 270x500 fp16x3')
    _report(stats, 'fp16x3_w48_270x500')
    assert 'conv_tt<fp16x3,k3,s1,8x32x96> split out' in stats and stats['bblockx3_fused split out']['ops'] >= 24
    _twin_rows(stats, *X3_TWIN_ROWS)


def test_every_launch_of_the_fp16x3_engine_w18_and_line_net(sncal, cuda):
    """The packaged hrnet_w18 (16 / 32 / 64 / 128 channels: by x3_shape_ok every 3x3 stride-1 convolution of stages 2-4 qualifies for the
    two-team kernel, and as no width is a multiple of 96 each runs alone on the 64 x 12 x 32 tile -- the 16- and 32-channel branches in one
    padded 64-channel block; stem, layer1, transitions, stride-2 and 1x1 convolutions on the generic split-arithmetic kernel) and the line
    network's head configuration."""
    from oracle import hrnet_ref as hr
    import width_cases as wc
    cfg = hr.load_config('hrnet_w18')
    sd = hr.seeded_state_dict(cfg, 3, 4.0)
    stats = verify_plan(sncal, cuda, 'hrnet_w18', sd, _frames(3, 135, 240, 22, cuda), 'fp16x3', tag='w18 135x240 fp16x3')
    _report(stats, 'fp16x3_w18_135x240')
    assert any(k.startswith('conv<fp16x3') for k in stats)
    # which kernel served the branch convolutions, by the schedule's own label
    x3n = sncal._lib.lib().sncal_x3_name().decode()
    wide = [e for e in stats['_case']['served'] if e['ksize'] == 3 and e['stride'] == 1 and '.stage' in e['name']]
    assert len(wide) == 2 * 2 * (2 + 3 + 4) and {e['cout'] for e in wide} == {16, 32, 64, 128}, len(wide)      # 2 blocks x 2 convolutions per branch
    for e in wide:
        want, alone = wc.expected_kernel('x3', x3n, e['cin'], e['cout'])
        assert e['kernel'] == want == f'conv_tt<{x3n},k3,s1,12x32x64>' and alone and e['members'] == 1, e
    sd = _weights('line_hrnet_w48')
    stats = verify_plan(sncal, cuda, 'line_hrnet_w48', sd, _frames(2, 540, 960, 23, cuda), 'fp16x3', tag='line w48 540p fp16x3')
    _report(stats, 'fp16x3_line_w48_540p')
    _twin_rows(stats, *X3_TWIN_ROWS)
