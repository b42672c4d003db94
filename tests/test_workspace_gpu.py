"""GPU: what happens BETWEEN the launches of an HRNet forward -- the workspace they share.

A forward is ~300 launches over one caller-provided workspace; tensors are carved out of it by a lifetime-based first-fit planner
(csrc/hrnet_layout.cpp) per (sub-batch, H, W), and the launch schedule (csrc/hrnet_schedule.cpp) is built per sub-batch size on top of
that layout.  tests/test_kernels_gpu.py checks every launch on the operands it read, and that a producer's bytes reach every reader;
this file checks what no single launch shows.  Every assertion is bit-exact equality of results the engine promises are equal:

  2a  the bytes the workspace held before a forward do not show in its results (nobody reads memory nobody wrote);
  2b  a ragged last sub-batch -- another schedule over the layout of the full sub-batch -- equals the same frames alone;
  2c  one handle driven through different shapes, outputs, input types, fp8 selections, taps and profiling modes equals fresh handles;
  3   a static audit of the planner over many shapes: two tensors that share bytes are never live in the same launch, and the forms the
      schedule reports per op (dense output, twin, helper in front) supply every reader of the op graph exactly once.
"""
import ctypes
import functools
import re

import numpy as np
import pytest
import torch

from oracle import hrnet_ref as hr

pytestmark = pytest.mark.gpu

ENGINES = [('hrnet_w48', 'fp16x3'), ('hrnet_w48', 'bf16'), ('hrnet_w48', 'fp8'), ('hrnet_w18', 'fp32'), ('hrnet_w18', 'fp16x3'),
           ('line_hrnet_w48', 'fp16x3'), ('line_hrnet_w48', 'bf16')]
ENGINE_IDS = [f'{c}-{d}' for c, d in ENGINES]
# (64, 96) the golden size; (96, 160) fused heads apply (half(H) is twice half(half(H))); (70, 122) odd: stem interpolation, unfused /
# split head, partial tiles in both directions; (135, 240) odd height
SIZES = [(64, 96), (96, 160), (70, 122), (135, 240)]
FILLS = (0x00, 0x3C, 0x7B, 0xFF)      # 0x7B..: a large finite value as fp32, bf16, fp16 and e4m3; 0xFF..: NaN in all four
DECODE = (540, 960)


@functools.lru_cache(maxsize=None)
def _state_dict(cfg_name):
    return hr.seeded_state_dict(hr.load_config(cfg_name), 3, 4.0)


def _keypoint_net(cfg_name):
    return not cfg_name.startswith('line_')


def _create(sncal, cuda, cfg_name, dtype):
    net = sncal.HRNetHeatmap(cfg_name, dtype=dtype, device=cuda)
    net.load_state_dict(_state_dict(cfg_name))
    return net


_SHARED = {}


def _shared(sncal, cuda, cfg_name, dtype):
    """One handle per network and engine for the whole module (W48's finalize is the dominant cost), created with no SNCAL_* variable set."""
    key = (cfg_name, dtype)
    if key not in _SHARED:
        _SHARED[key] = _create(sncal, cuda, cfg_name, dtype)
    return _SHARED[key]


def _frames(B, H, W, seed, cuda):
    return hr.seeded_input(B, H, W, seed).to(cuda)


def _forward(net, x, want_heat=True, want_kpts=None):
    """(heat, kpts) clones; keypoints on the keypoint networks unless told otherwise."""
    kp = _keypoint_net_of(net) if want_kpts is None else want_kpts
    heat, kpts = net.forward(x, want_heat=want_heat, decode_size=DECODE if kp else None)
    torch.cuda.synchronize()
    return (None if heat is None else heat.clone()), (None if kpts is None else kpts.clone())


def _keypoint_net_of(net):
    return net.cfg.get('head', 'logsoftmax') == 'logsoftmax'


def _bits(t):
    return t.view(torch.int32)


def _same(a, b):
    """Bit for bit (NaN-safe), None == None."""
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _family(label):
    """A profile label with its tile parameters stripped: conv<bf16,k3,s1,NI3,MI6,G4> -> conv<bf16,k3,s1>."""
    return re.sub(r',(NI\d+|MI\d+|G\d+|\d+x\d+x\d+)', '', label)


def _launch_labels(net, x):
    """Full labels of the launches of one profiled forward of x.  Only the op that LEADS a launch is read: the executor labels that op alone
    and never clears a label, so a grouped member or the second op of a fused pair may still carry the label of a launch that covered it at
    another shape."""
    net.set_profiling(1)
    _forward(net, x)
    labels, prev = set(), -1
    for o in net.plan_ops():
        if not o['active']:
            continue
        assert o['launch'] >= 0, o['idx']
        if o['launch'] != prev:
            if o['kernel']:
                labels.add(o['kernel'])
        prev = o['launch']
    net.set_profiling(0)
    return labels


def _labels(net, x):
    return {_family(k) for k in _launch_labels(net, x)}


# ---- coverage condition ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cfg_name,dtype', ENGINES, ids=ENGINE_IDS)
def test_small_sizes_reach_every_kernel_family_of_the_540p_plan(sncal, cuda, cfg_name, dtype):
    """The four small sizes of this module (batch 3) run, per engine, every kernel family -- profile label with the tile parameters
    stripped -- that the engine's 540x960 batch-3 plan runs; no further size had to be added."""
    net = _shared(sncal, cuda, cfg_name, dtype)
    if dtype == 'fp8':
        net.calibrate_fp8(_frames(3, 96, 160, 40, cuda))
        net.set_fp8_layers('all')
    want = _labels(net, _frames(3, 540, 960, 41, cuda))
    got = set()
    for H, W in SIZES:
        got |= _labels(net, _frames(3, H, W, 42, cuda))
    net._ws = None              # (the 540p workspace: the tests below size their own)
    print('KERNEL-FAMILIES', cfg_name, dtype, sorted(got))
    assert want <= got, f'families of the 540p plan no small size reaches: {sorted(want - got)}'


# ---- 2a: workspace contents do not show -----------------------------------------------------------------------------
@pytest.mark.parametrize('hw', SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('cfg_name,dtype', ENGINES, ids=ENGINE_IDS)
def test_workspace_contents_do_not_show_in_the_results(sncal, cuda, cfg_name, dtype, hw):
    """The same forward over a workspace filled with 0x00, 0x3C, 0x7B (large finite in every storage type) and 0xFF (NaN in every
    storage type) bytes: heat and keypoints bit-identical, fp16x3 range counters zero.  A difference is a launch that reads memory
    nobody wrote -- a dead lane computing garbage x 0 is one NaN pattern away from a poisoned heatmap (x3.hpp X3_SPLIT1)."""
    net = _shared(sncal, cuda, cfg_name, dtype)
    x = _frames(3, hw[0], hw[1], 50, cuda)
    if dtype == 'fp8':
        net.calibrate_fp8(x)
        net.set_fp8_layers('all')
    net.range_status(clear=True)
    results = []
    for fill in FILLS:
        ws = net._workspace(3, hw[0], hw[1])
        ws.fill_(fill)
        assert ws is net._ws
        results.append(_forward(net, x))
        assert net.range_status(clear=True) == (0, 0), f'range counters after the 0x{fill:02X} fill'
    heat0, kp0 = results[0]
    assert not torch.isnan(heat0).any()
    for fill, (heat, kp) in zip(FILLS[1:], results[1:]):
        assert _same(heat, heat0), f'heat differs between the 0x00 and the 0x{fill:02X} fill: {int((_bits(heat) != _bits(heat0)).sum())} elements'
        assert _same(kp, kp0), f'keypoints differ between the 0x00 and the 0x{fill:02X} fill'


# ---- 2b: a ragged tail equals the same frames alone ---------------------------------------------------------------
_SUB4 = {}


@pytest.mark.parametrize('cfg_name,dtype', ENGINES, ids=ENGINE_IDS)
def test_ragged_last_sub_batch_equals_the_same_frames_alone(sncal, cuda, monkeypatch, cfg_name, dtype):
    """SNCAL_SUBBATCH=4, B = 7 (4 + 3) and B = 5 (4 + 1) at 96x160 and 70x122: the tail runs the schedule of 3 / 1 frames over the layout
    laid out for 4.  Every frame's heat and keypoints (also keypoints alone, the decode-fused path) equal those of a handle created
    without the variable that runs the frame's own sub-batch alone -- its own layout, its own schedule."""
    key = (cfg_name, dtype)
    if key not in _SUB4:
        monkeypatch.setenv('SNCAL_SUBBATCH', '4')
        _SUB4[key] = _create(sncal, cuda, cfg_name, dtype)
        monkeypatch.delenv('SNCAL_SUBBATCH')
    net4, alone = _SUB4[key], _shared(sncal, cuda, cfg_name, dtype)
    modes = [True, False] if _keypoint_net(cfg_name) else [True]
    for H, W in ((96, 160), (70, 122)):
        for B in (7, 5):
            x = _frames(B, H, W, 60 + B, cuda)
            if dtype == 'fp8':
                for n in (net4, alone):
                    n.calibrate_fp8(x)
                    n.set_fp8_layers('all')
            for want_heat in modes:
                heat, kp = _forward(net4, x, want_heat=want_heat)
                assert net4.plan_tensor(0)['sub_batch'] == 4
                for lo, hi in ((0, 4), (4, B)):
                    h1, k1 = _forward(alone, x[lo:hi].contiguous(), want_heat=want_heat)
                    what = f'{H}x{W} B={B} frames {lo}:{hi} want_heat={want_heat}'
                    assert _same(None if heat is None else heat[lo:hi], h1), 'heat ' + what
                    assert _same(None if kp is None else kp[lo:hi], k1), 'keypoints ' + what


# ---- 2c: one handle, many calls -------------------------------------------------------------------------------------
CALLS = ('A', 'B', 'C', 'A u8', 'A again')
_SEQ = {}


def _sequence(sncal, cuda, cfg_name, dtype):
    """One handle per engine driven through A = (3, 96, 160) heat + keypoints; B = (1, 70, 122) keypoints only; C = (5, 135, 240) heat
    only; A from uint8 frames (exact k/255 values); A again -- layouts cached and dropped, schedules rebuilt, ticket words reused, a
    workspace that only grows.  (The line networks have no keypoint decode: their B call returns the heatmap.)  Run once per engine."""
    key = (cfg_name, dtype)
    if key not in _SEQ:
        kp_net = _keypoint_net(cfg_name)
        gen = torch.Generator().manual_seed(70)
        a_u8 = torch.randint(0, 256, (3, 96, 160, 3), dtype=torch.uint8, generator=gen)
        xa = a_u8.permute(0, 3, 1, 2).contiguous().to(torch.float32).div(255).to(cuda)
        a_kw = dict(want_heat=True, want_kpts=kp_net)
        calls = {'A': (xa, a_kw), 'B': (_frames(1, 70, 122, 71, cuda), dict(want_heat=not kp_net, want_kpts=kp_net)),
                 'C': (_frames(5, 135, 240, 72, cuda), dict(want_heat=True, want_kpts=False)), 'A u8': (a_u8.to(cuda), a_kw),
                 'A again': (xa, a_kw)}

        def prepared():
            n = _create(sncal, cuda, cfg_name, dtype)
            if dtype == 'fp8':
                n.calibrate_fp8(xa)
                n.set_fp8_layers('all')
            return n

        net = prepared()
        _SEQ[key] = (net, calls, {name: _forward(net, *calls[name][:1], **calls[name][1]) for name in CALLS}, prepared)
    return _SEQ[key]


@pytest.mark.parametrize('call', CALLS[:4])
@pytest.mark.parametrize('cfg_name,dtype', ENGINES, ids=ENGINE_IDS)
def test_one_handle_through_many_calls_equals_a_fresh_handle(sncal, cuda, cfg_name, dtype, call):
    """Each call of the sequence on the used handle equals, bit for bit, the same call on a handle that has done nothing else."""
    net, calls, got, prepared = _sequence(sncal, cuda, cfg_name, dtype)
    x, kw = calls[call]
    h1, k1 = _forward(prepared(), x, **kw)
    assert _same(got[call][0], h1) and _same(got[call][1], k1), f'call {call} on the used handle differs from a fresh handle'


@pytest.mark.parametrize('cfg_name,dtype', ENGINES, ids=ENGINE_IDS)
def test_one_handle_returns_to_the_same_bits(sncal, cuda, cfg_name, dtype):
    """The three A results of the sequence equal each other (fp32 frames, uint8 frames, fp32 again after other shapes); fp8 layer
    selections 'all' -> 'stage4,c192' -> 'all' come back to the first bits; taps registered and cleared, profiling 1 and 0 change nothing."""
    net, calls, got, _ = _sequence(sncal, cuda, cfg_name, dtype)
    xa, kw = calls['A']
    first = got['A']
    for name in ('A u8', 'A again'):
        assert _same(got[name][0], first[0]) and _same(got[name][1], first[1]), f'call {name} differs from the first A'
    if dtype == 'fp8':
        net.set_fp8_layers('stage4,c192')
        other = _forward(net, xa, **kw)
        assert not _same(other[0], first[0])                       # (the selection does something)
        net.set_fp8_layers('all')
        back = _forward(net, xa, **kw)
        assert _same(back[0], first[0]) and _same(back[1], first[1]), "fp8 layers 'all' -> 'stage4,c192' -> 'all'"
    net.workspace_bytes(3, 96, 160)
    tapped = [net.tap(o['idx'], o['out']) for o in net.plan_ops() if o['active'] and o['type'] == 'conv'][:8]
    assert len(tapped) == 8
    with_taps = _forward(net, xa, **kw)
    net.clear_taps()
    cleared = _forward(net, xa, **kw)
    net.set_profiling(1)
    profiled = _forward(net, xa, **kw)
    net.set_profiling(0)
    plain = _forward(net, xa, **kw)
    for name, r in (('taps registered', with_taps), ('taps cleared', cleared), ('profiling 1', profiled), ('profiling 0', plain)):
        assert _same(r[0], first[0]) and _same(r[1], first[1]), name
    assert net.range_status(clear=True) == (0, 0)


# ---- 3: static audit of the planner ----------------------------------------------------------------------------------
AUDIT_B = (1, 2, 3, 8, 64, 67)
AUDIT_HW = [(H, H + 37) for H in range(32, 161, 3)] + [(270, 480), (540, 960), (1080, 1920), (270, 500), (140, 240)]
AUDIT_ENV = (None, 'SNCAL_FUSED_HEAD', 'SNCAL_CONV_TT', 'SNCAL_FUSE_BBLOCK', 'SNCAL_FUSE_BNECK')
FP8_SELECTIONS = ('all', 'stage4', 'c96', 'none')


class _Plan:
    """The plan of a handle as plain arrays, read through the C ABI (the op graph once, what the layout decides per layout)."""

    def __init__(self, net):
        self.net, self.L, self.h = net, net._L, net._h
        from sncal_amd import _lib
        self.po, self.pt = _lib.PlanOp(), _lib.PlanTensor()
        self.n_ops = self.L.sncal_hrnet_plan_num_ops(self.h)
        self.n_t = self.L.sncal_hrnet_plan_num_tensors(self.h)
        self.static = None

    def read(self):
        L, h, po, pt = self.L, self.h, self.po, self.pt
        rpo, rpt = ctypes.byref(po), ctypes.byref(pt)
        if self.static is None:
            self.static = []
            for i in range(self.n_ops):
                assert L.sncal_hrnet_plan_op(h, i, rpo) == 0
                reads = [po.in_, po.res, po.base, po.head_direct] + list(po.src)[:po.nsrc] + list(po.head_src)[:po.head_nsrc] + \
                    list(po.head_fold)[:po.head_nfold]
                self.static.append((po.type, po.in_, po.res, po.out, tuple(t for t in reads if t >= 0)))
        dyn = []
        for i in range(self.n_ops):
            assert L.sncal_hrnet_plan_op(h, i, rpo) == 0
            if po.active:
                dyn.append((i, po.launch, po.fp8, po.res_twin, po.writes_out, po.writes_twin, po.prep_in))
        tens = np.zeros((self.n_t, 6), dtype=np.int64)           # alive, offset, bytes, twin, first, last
        for t in range(self.n_t):
            assert L.sncal_hrnet_plan_tensor(h, t, rpt) == 0
            tens[t] = (pt.alive, pt.offset, pt.bytes, pt.twin, pt.first, pt.last)
        return dyn, tens


def _audit_layout(plan, ws_bytes, what, tamper=None):
    """Hazards from the op fields alone.  Per launch: read = in, res, base, src[], head_direct, head_src[], head_fold[] of its ops, the twin
    beside the tensor where the op's fp8 field (e4m3 / split two-team convolution: `in`) or res_twin (`res`) says so, minus what the launch
    itself produces (a fused pair's intermediate); written = each out, plus its twin where the plan shows one alive.  A tensor's interval
    runs from its first writing launch to its last reading (or writing) launch.  The allocator's own first / last are only printed."""
    dyn, tens = plan.read()
    if tamper is not None:
        tamper(dyn, tens)
    alive, off, nbytes, twin = tens[:, 0] != 0, tens[:, 1], tens[:, 2], tens[:, 3]
    n_t = len(tens)
    lo = np.full(n_t, -1, dtype=np.int64)
    hi = np.full(n_t, -1, dtype=np.int64)
    by_launch = {}
    for i, launch, fp8, res_twin, *_ in dyn:
        assert launch >= 0, f'{what}: active op {i} is covered by no launch'
        by_launch.setdefault(launch, []).append((i, fp8, res_twin))
    for launch in sorted(by_launch):
        written, read = set(), set()
        for i, fp8, res_twin in by_launch[launch]:
            typ, t_in, t_res, t_out, reads = plan.static[i]
            read.update(reads)
            if typ == 1 and fp8 in (1, 2) and t_in >= 0 and twin[t_in] >= 0:
                assert alive[twin[t_in]], f'{what}: op {i} reads the twin of tensor {t_in}, which is not allocated'
                read.add(int(twin[t_in]))
            if res_twin:
                assert twin[t_res] >= 0 and alive[twin[t_res]], f'{what}: op {i} reads the twin of its residual {t_res}, which is not allocated'
                read.add(int(twin[t_res]))
            if t_out >= 0:
                written.add(t_out)
                if twin[t_out] >= 0 and alive[twin[t_out]]:
                    written.add(int(twin[t_out]))
        read -= written                                   # produced and consumed inside the same (fused) launch
        for t in read:
            assert alive[t], f'{what}: launch {launch} reads tensor {t}, which is not allocated'
            assert 0 <= lo[t] < launch, f'{what}: launch {launch} reads tensor {t}, which no earlier launch wrote (first writer {lo[t]})'
            hi[t] = max(hi[t], launch)
        for t in written:
            assert alive[t], f'{what}: launch {launch} writes tensor {t}, which is not allocated'
            if lo[t] < 0:
                lo[t] = launch
            hi[t] = max(hi[t], launch)
    used = np.nonzero(alive)[0]
    assert (lo[used] >= 0).all(), f'{what}: allocated tensors no launch writes: {used[lo[used] < 0].tolist()}'
    end = off[used] + nbytes[used]
    assert (end <= ws_bytes).all(), f'{what}: tensors {used[end > ws_bytes].tolist()} end beyond the {ws_bytes} bytes sncal_hrnet_workspace returned'
    share = (off[used][:, None] < end[None, :]) & (off[used][None, :] < end[:, None])
    apart = (hi[used][:, None] < lo[used][None, :]) | (hi[used][None, :] < lo[used][:, None])
    clash = np.argwhere(np.triu(share & ~apart, 1))
    if len(clash):
        a, b = (int(used[k]) for k in clash[0])
        raise AssertionError(f'{what}: {len(clash)} pairs of tensors share bytes while both live; first: tensor {a} [{off[a]}, {off[a] + nbytes[a]}) '
                             f'launches {lo[a]}..{hi[a]} (allocator ops {tens[a, 4]}..{tens[a, 5]}) and tensor {b} [{off[b]}, {off[b] + nbytes[b]}) '
                             f'launches {lo[b]}..{hi[b]} (allocator ops {tens[b, 4]}..{tens[b, 5]})')
    _audit_forms(plan, dyn, alive, twin, what)


def _audit_forms(plan, dyn, alive, twin, what):
    """The forms the schedule reports per op -- writes_out, writes_twin, prep_in (include/sncal.h) -- against the op graph alone.  A reduced-
    precision convolution (fp8 field 1 / 2) reads the twin of `in`, a res_twin convolution the twin of `res`, everybody else the dense
    tensors.  A read inside the launch that produces the tensor (a fused pair's intermediate) needs no form at all.
      1  a twin that is read was written by an earlier launch, or made by a helper in front of that launch or an earlier one (a dense
         tensor that is read has an earlier writer: _audit_layout; that the writer wrote the dense form: 4);
      2  for every twin read by another launch, exactly one of: a producer of the tensor reports writes_twin, EVERY launch reading it as
         `in` reports prep_in -- never both;
      3  an op that writes neither form is the first op of a two-op launch whose second op reads its output;
      4  every producer of a tensor reports writes_out when a later launch reads the dense form;
      5  no launch of a stock network has split_f32 in front (prep_in == 2): the split engine's producers write every twin."""
    producers, in_readers, members = {}, {}, {}
    for d in dyn:
        i, launch, fp8 = d[:3]
        typ, t_in, _, t_out, _ = plan.static[i]
        members.setdefault(launch, []).append(i)
        if t_out >= 0:
            producers.setdefault(t_out, []).append(d)
        if typ == 1 and fp8 in (1, 2) and t_in >= 0 and twin[t_in] >= 0:
            in_readers.setdefault(t_in, []).append(d)

    def local(t, launch):
        return any(p[1] == launch for p in producers.get(t, ()))

    for t, rs in in_readers.items():                                                                  # 2
        rs = [r for r in rs if not local(t, r[1])]
        by_producer = any(p[5] for p in producers.get(t, ()))
        front = [r[0] for r in rs if r[6]]
        assert not (by_producer and front), f'{what}: twin of tensor {t}: both written by its producer and made in front of op(s) {front}'
        assert by_producer or len(front) == len(rs), \
            f'{what}: twin of tensor {t}: its producer does not write it and no helper makes it in front of op(s) {[r[0] for r in rs if not r[6]]}'
    for i, launch, fp8, res_twin, w_out, w_twin, prep in dyn:
        typ, t_in, t_res, t_out, reads = plan.static[i]
        dense, twins = list(reads), []
        if typ == 1 and fp8 in (1, 2) and t_in >= 0 and twin[t_in] >= 0 and not prep:      # (with a helper in front: `in` itself, dense)
            dense.remove(t_in)
            twins.append(t_in)
        if res_twin:
            dense.remove(t_res)
            twins.append(t_res)
        for t in twins:                                                                               # 1
            assert local(t, launch) or any(p[5] and p[1] < launch for p in producers.get(t, ())) or \
                any(r[6] and r[1] <= launch for r in in_readers.get(t, ())), \
                f'{what}: op {i} (launch {launch}) reads the twin of tensor {t}, which no earlier launch wrote and no helper made'
        for t in dense:                                                                               # 4
            for p in producers.get(t, ()):
                assert p[1] >= launch or p[4], f'{what}: op {p[0]} does not write tensor {t} in dense form, which op {i} (launch {launch}) reads'
        if w_twin:
            assert t_out >= 0 and twin[t_out] >= 0 and alive[twin[t_out]], f'{what}: op {i} writes the twin of tensor {t_out}, which is not allocated'
    for i, launch, _, _, w_out, w_twin, _ in dyn:                                                     # 3
        t_out = plan.static[i][3]
        if t_out >= 0 and not w_out and not w_twin:
            pair = members[launch]
            assert len(pair) == 2 and pair[0] == i and t_out in plan.static[pair[1]][4], \
                f'{what}: op {i} writes neither form of tensor {t_out} and is not the first op of a fused pair that reads it'
    split_front = [d[0] for d in dyn if d[6] == 2]                                                    # 5
    assert not split_front, f'{what}: split_f32 in front of op(s) {split_front}: a stock network has none'


def _audit(net, what):
    plan = _Plan(net)
    seen = set()
    for B in AUDIT_B:
        for H, W in AUDIT_HW:
            ws_bytes = net.workspace_bytes(B, H, W)
            key = (net.plan_tensor(0)['sub_batch'], H, W)
            if key in seen:                               # (B = 67 lays out the 64 frames of its first sub-batch)
                continue
            seen.add(key)
            _audit_layout(plan, ws_bytes, f'{what} B={B} {H}x{W}')
    print('LAYOUTS-AUDITED', what, len(seen))
    assert len(seen) >= 200
    return len(seen)


@pytest.mark.parametrize('cfg_name,dtype', [('hrnet_w48', 'fp16x3'), ('hrnet_w48', 'bf16')], ids=['hrnet_w48-fp16x3', 'hrnet_w48-bf16'])
def test_the_audit_reports_what_a_wrong_planner_would_do(sncal, cuda, cfg_name, dtype):
    """The audit's own failure paths, on a real plan edited in Python (the planner's stretched lifetimes make such layouts impossible, so
    they cannot be seen otherwise): the output of a fused pair placed on the first op's input -- what placing it after that input's release
    can do --, the same for a grouped launch's members, and a tensor that ends beyond the workspace."""
    net = _shared(sncal, cuda, cfg_name, dtype)
    ws_bytes = net.workspace_bytes(3, 96, 160)
    plan = _Plan(net)
    _audit_layout(plan, ws_bytes, 'untouched')
    dyn, _ = plan.read()
    by_launch = {}
    for i, launch, *_ in dyn:
        by_launch.setdefault(launch, []).append(i)
    fused = [ops for ops in by_launch.values() if len(ops) == 2 and plan.static[ops[0]][3] in plan.static[ops[1]][4]]
    grouped = [ops for ops in by_launch.values() if len(ops) >= 2 and plan.static[ops[0]][3] not in plan.static[ops[1]][4]]
    assert fused and grouped
    for ops in (fused[0], fused[-1], grouped[0], grouped[-1]):
        t_in, t_out = plan.static[ops[0]][1], plan.static[ops[-1]][3]

        def onto_input(dyn, tens, t_in=t_in, t_out=t_out):
            small, large = (t_in, t_out) if tens[t_in, 2] <= tens[t_out, 2] else (t_out, t_in)
            tens[small, 1] = tens[large, 1]              # (the smaller one into the larger one's slot: stays inside the workspace)

        with pytest.raises(AssertionError, match='share bytes while both live'):
            _audit_layout(plan, ws_bytes, 'tampered', onto_input)

    def beyond(dyn, tens):
        t = int(np.nonzero(tens[:, 0])[0][-1])
        tens[t, 1] = ws_bytes - tens[t, 2] + 256

    with pytest.raises(AssertionError, match='end beyond'):
        _audit_layout(plan, ws_bytes, 'tampered', beyond)

    def setting(k, field, value):                       # row k of the plan's per-op report with one field edited
        def tamper(dyn, tens):
            row = list(dyn[k])
            row[field] = value
            dyn[k] = tuple(row)
        return tamper

    W_OUT, W_TWIN, PREP = 4, 5, 6
    row_of_out = {plan.static[d[0]][3]: k for k, d in enumerate(dyn)}
    dense_read = [row_of_out[t] for d in dyn for t in plan.static[d[0]][4]
                  if not (d[2] in (1, 2) and t == plan.static[d[0]][1]) and not (d[3] and t == plan.static[d[0]][2])
                  and t in row_of_out and dyn[row_of_out[t]][1] < d[1]]
    assert dense_read and dyn[dense_read[0]][W_OUT]
    with pytest.raises(AssertionError, match='does not write tensor .* in dense form'):
        _audit_layout(plan, ws_bytes, 'tampered', setting(dense_read[0], W_OUT, 0))
    if dtype == 'fp16x3':                               # (the bf16 engine has no twins)
        handed = [(row_of_out[plan.static[d[0]][1]], k) for k, d in enumerate(dyn)
                  if d[2] == 2 and dyn[row_of_out[plan.static[d[0]][1]]][W_TWIN] and dyn[row_of_out[plan.static[d[0]][1]]][1] < d[1]]
        assert handed
        producer, reader = handed[0]
        with pytest.raises(AssertionError, match='its producer does not write it'):
            _audit_layout(plan, ws_bytes, 'tampered', setting(producer, W_TWIN, 0))
        with pytest.raises(AssertionError, match='both written by its producer'):
            _audit_layout(plan, ws_bytes, 'tampered', setting(reader, PREP, 2))


_AUDIT_CASES = [(c, d, e) for c, d in ENGINES for e in AUDIT_ENV]
# which switch changes the launches of which network and engine (the kernels its default 540p plan runs: head_fused / headx3_fused,
# conv_tt, bblock48_fused, bneck_*_x3); elsewhere the switch is read and changes nothing
SWITCH_APPLIES = {
    ('hrnet_w48', 'fp16x3'): {'SNCAL_FUSED_HEAD', 'SNCAL_CONV_TT', 'SNCAL_FUSE_BNECK'},
    ('hrnet_w48', 'bf16'): {'SNCAL_FUSED_HEAD', 'SNCAL_CONV_TT', 'SNCAL_FUSE_BBLOCK'},
    ('hrnet_w48', 'fp8'): {'SNCAL_FUSED_HEAD', 'SNCAL_CONV_TT', 'SNCAL_FUSE_BBLOCK'},
    ('hrnet_w18', 'fp32'): set(),
    ('hrnet_w18', 'fp16x3'): {'SNCAL_CONV_TT'},
    ('line_hrnet_w48', 'fp16x3'): {'SNCAL_CONV_TT', 'SNCAL_FUSE_BNECK'},
    ('line_hrnet_w48', 'bf16'): {'SNCAL_FUSED_HEAD', 'SNCAL_CONV_TT', 'SNCAL_FUSE_BBLOCK'},
}
_DEFAULT_LABELS = {}


def _labels_540p(net, cuda):
    return _launch_labels(net, _frames(1, 540, 960, 81, cuda))


@pytest.mark.parametrize('cfg_name,dtype,env', _AUDIT_CASES, ids=[f'{c}-{d}-{e or "default"}' for c, d, e in _AUDIT_CASES])
def test_planner_never_overlaps_two_live_tensors(sncal, cuda, monkeypatch, cfg_name, dtype, env):
    """The audit computes layouts only and launches nothing: sub-batches of 1, 2, 3, 8 and 64 frames (B = 67 lays out 64), H in
    range(32, 161, 3) with W = H + 37 and five larger sizes, the default network and one network per switch that changes the schedule (fused
    head, two-team kernel, fused BasicBlock, fused Bottleneck seams off).  That a switch took effect is checked first, with one profiled
    540x960 frame: the launch labels differ from the default network's exactly where the switch applies (SWITCH_APPLIES)."""
    default = _shared(sncal, cuda, cfg_name, dtype)
    if env is None:
        net = default
    else:
        monkeypatch.setenv(env, '0')
        net = _create(sncal, cuda, cfg_name, dtype)
        monkeypatch.delenv(env)
    for n in {id(default): default, id(net): net}.values():
        if dtype == 'fp8':
            n.calibrate_fp8(_frames(1, 64, 96, 80, cuda))
            n.set_fp8_layers('all')
    if env is not None:
        if (cfg_name, dtype) not in _DEFAULT_LABELS:
            _DEFAULT_LABELS[(cfg_name, dtype)] = _labels_540p(default, cuda)
            default._ws = None
        changed = _labels_540p(net, cuda) != _DEFAULT_LABELS[(cfg_name, dtype)]
        assert changed == (env in SWITCH_APPLIES[(cfg_name, dtype)]), f'{env}=0 changed the launch labels: {changed}'
    _audit(net, f'{cfg_name} {dtype} {env + "=0" if env else "default"}')
    net._ws = None


@pytest.mark.parametrize('selection', FP8_SELECTIONS[1:])
def test_planner_never_overlaps_two_live_tensors_fp8_selections(sncal, cuda, selection):
    """The e4m3 twins live only while a selected layer reads them: the same audit under the other layer selections ('all' is the case above)."""
    net = _shared(sncal, cuda, 'hrnet_w48', 'fp8')
    net.calibrate_fp8(_frames(1, 64, 96, 80, cuda))
    try:
        net.set_fp8_layers(selection)
        _audit(net, f'hrnet_w48 fp8 layers {selection}')
    finally:
        net.set_fp8_layers('all')


def test_a_calibrated_fp8_handle_can_be_calibrated_again(sncal, cuda):
    """At the C ABI: calibrate, forward, ask sncal_hrnet_calibrate_fp8_workspace for the size of the next calibration (more than the fp8
    layout's at this shape: the calibration forward has no e4m3 twins and another first-fit geometry), calibrate again in exactly that many
    bytes -- and the query has dropped the layout, as the header says: plan_tensor refuses until the next workspace query."""
    from sncal_amd import _lib
    L = _lib.lib()
    net = _create(sncal, cuda, 'hrnet_w48', 'fp8')
    x = _frames(3, 64, 96, 90, cuda)
    net.calibrate_fp8(x)
    net.set_fp8_layers('all')
    first = _forward(net, x)
    n_fp8 = net.workspace_bytes(3, 64, 96)
    n = ctypes.c_size_t()
    _lib.check(L.sncal_hrnet_calibrate_fp8_workspace(net._h, 3, 64, 96, ctypes.byref(n)), 'sncal_hrnet_calibrate_fp8_workspace')
    assert n.value > 0
    print('CALIBRATION-WORKSPACE', n.value, 'fp8 layout', n_fp8)
    with pytest.raises(_lib.SncalError):
        net.plan_tensor(0)
    ws = torch.empty(n.value, dtype=torch.uint8, device=cuda)
    _lib.check(L.sncal_hrnet_calibrate_fp8(net._h, x.data_ptr(), 3, 64, 96, ws.data_ptr(), ws.numel(), _lib.current_stream_ptr()),
               'sncal_hrnet_calibrate_fp8')
    torch.cuda.synchronize()
    again = _forward(net, x)
    assert _same(again[0], first[0]) and _same(again[1], first[1])          # same frames, same ranges, same bits
