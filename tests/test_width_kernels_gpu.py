"""GPU: every launch of the width families beyond W18 / W32 / W48 (tests/width_cases.py) against torch fp32, and which kernel served what.

The instrument is tests/test_kernels_gpu.py's verify_plan, unchanged tolerances: it taps every op of a real forward and recomputes it from the
operands that launch read.  The networks are tiny (reduced depth, 3 frames of 72x104: branch maps 18x26 / 9x13 / 5x7 / 3x4, head 36x52 --
every 32-column tile partial, partial rows in the 8-, 12- and 4-row tiles, three stacked frames of 3 + 1 rows inside one 12-row tile), but
their WIDTHS take the code paths no packaged config reaches:

    split engine   64-channel blocks with a partial last block behind full ones (80, 144, 160, 400), the 48-channel last block at nb > 0
                   (112, 176, 240), odd counts of 16-channel input stages (5 .. 25), 3 and 5 blocks of 96 (288, 480)
    bf16 / fp8     3 and 5 blocks of 96, e4m3 stage counts 5 and 8 with a half-empty last stage (cin 288, 480)
    every engine   the cout <= 480 refusal (512, 576 on the generic kernel; on the split engine its epilogue writes the split twin),
                   the 288 + 480 = 768-channel group that must not share one launch, generic variants at 5 .. 36 output fragments

Every case asserts, from the schedule's own labels (plan_ops()['kernel'] through verify_plan's `served` list), that each 3x3 stride-1
convolution of stages 2-4 ran on the kernel the predicates of conv_tt.hpp name for its width (width_cases.expected_kernel), and that no
active conv op went unchecked.
"""
import pytest

from test_kernels_gpu import _frames, _report, _twin_rows, verify_plan, X3_TWIN_ROWS
import width_cases as wc

pytestmark = pytest.mark.gpu

_SD = {}


def _weights(name):
    """bench.seeded_weights of the reduced-depth network, made once per family."""
    if name not in _SD:
        import bench
        _SD[name] = bench.seeded_weights(wc.reduced(name), seed=1)
    return _SD[name]


def _x3_name(sncal):
    return sncal._lib.lib().sncal_x3_name().decode()


def _served_as_the_predicates_say(sncal, stats, dtype, fp8_layers=None, tile96=None):
    """Each 3x3 stride-1 convolution of stages 2-4: label by width.  tile96: the tile a split-engine launch of 96-channel blocks must name."""
    c = stats['_case']
    assert c['conv_ops_checked'] == c['conv_ops_active'] > 0, (c['conv_ops_checked'], c['conv_ops_active'])
    engine = {'fp16x3': 'x3', 'bf16x3': 'x3', 'x3': 'x3'}.get(dtype, dtype)
    x3n = _x3_name(sncal)
    widths = [int(t[1:]) for t in (fp8_layers or '').split(',') if t.startswith('c')]
    by_width = {}
    n = 0
    for e in c['served']:
        if e['ksize'] != 3 or e['stride'] != 1 or '.stage' not in e['name']:
            continue
        n += 1
        sel = engine == 'fp8' and (fp8_layers == 'all' or e['cout'] in widths)
        want, alone = wc.expected_kernel(engine, x3n, e['cin'], e['cout'], fp8=sel)
        assert e['kernel'].startswith(want), (e['name'], e['cin'], e['cout'], e['kernel'], want)
        assert e['fp8'] == e['kernel'].startswith('conv_tt<fp8'), e
        if engine == 'x3' and want.startswith('conv_tt') and not alone:
            assert e['kernel'].endswith('x32x96>'), e
            if tile96:
                assert e['kernel'] == f'conv_tt<{x3n},k3,s1,{tile96}>', (e['kernel'], tile96)
        if alone:
            assert e['members'] == 1, e
        by_width.setdefault(e['cout'], set()).add(e['kernel'])
    assert n >= 18, n                       # 2 + 3 + 4 branches x 2 convolutions of a BasicBlock
    c['kernel_by_width'] = {str(w): sorted(k) for w, k in sorted(by_width.items())}
    return c['kernel_by_width']


def _run(sncal, cuda, monkeypatch, name, dtype, fp8_layers=None, frames=(3, 72, 104), seed=31, small_items=None, tile96=None):
    if small_items is not None:
        monkeypatch.setenv('SNCAL_TT_SMALL_ITEMS', small_items)
    tag = f"{name} {frames[1]}x{frames[2]}x{frames[0]} {dtype}" + (f' {fp8_layers}' if fp8_layers else '') + (f' small {small_items}' if small_items else '')
    stats = verify_plan(sncal, cuda, wc.reduced(name), _weights(name), _frames(*frames, seed, cuda), dtype, fp8_layers=fp8_layers, tag=tag)
    kinds = _served_as_the_predicates_say(sncal, stats, dtype, fp8_layers, tile96)
    _report(stats, 'widths_' + tag.replace(' ', '_').replace(',', '_'))
    if dtype == 'fp16x3':
        _twin_rows(stats, *X3_TWIN_ROWS)
    return stats, kinds


def _no_fp8_launch(stats):
    c = stats['_case']
    assert not any(k.startswith('conv_tt<fp8') for k in stats), sorted(stats)
    assert not any(k.startswith('conv_tt<fp8') for k in c['profile_launches']), sorted(c['profile_launches'])
    assert not any(e['fp8'] for e in c['served'])
    assert c['twin_pairs_compared'] == c['twin_pairs_expected'] == 0, c         # nothing reads an e4m3 twin


@pytest.mark.parametrize('dtype', ['fp16x3', 'bf16', 'fp32', 'fp8'])
def test_every_launch_w64(sncal, cuda, monkeypatch, dtype):
    """64 / 128 / 256 / 512, the reference's hrnet_w64 family.  Split engine: 1, 2 and 4 full 64-channel blocks on the 64 x 12 x 32 tile, each
    launched alone; 512 > 480 on the generic split kernel, whose epilogue writes the split twin.  bf16: no width is a multiple of 96, so
    every convolution runs on the generic kernel -- and so does the fp8 engine with 'all': calibration and forward run, every launch is
    checked, no conv_tt<fp8 row appears."""
    stats, kinds = _run(sncal, cuda, monkeypatch, 'W64', dtype, fp8_layers='all' if dtype == 'fp8' else None)
    if dtype == 'fp16x3':
        assert kinds['64'] == kinds['128'] == kinds['256'] == ['conv_tt<fp16x3,k3,s1,12x32x64>'.replace('fp16x3', _x3_name(sncal))], kinds
        assert all(k.startswith('conv<') for k in kinds['512']), kinds
        assert any(k.startswith('conv<') and k.endswith(' split out') for k in stats), sorted(stats)       # the generic epilogue's twin
    if dtype == 'fp8':
        _no_fp8_launch(stats)


@pytest.mark.parametrize('dtype', ['fp16x3', 'bf16', 'fp32'])
def test_every_launch_p64(sncal, cuda, monkeypatch, dtype):
    """80 / 112 / 176 / 240.  Split engine: 80 = 64 + 16 (a partial last block behind a full one), 112 / 176 / 240 = 1, 2, 3 full blocks + the
    48-channel last block (the epilogue's narrow48 path at nb = 1, 2, 3); 5 / 7 / 11 / 15 input stages of 16 channels.  bf16 / fp32: the
    generic kernel at 5, 7, 11 and 15 output fragments."""
    stats, kinds = _run(sncal, cuda, monkeypatch, 'P64', dtype)
    assert sorted(kinds) == ['112', '176', '240', '80'], kinds


@pytest.mark.parametrize('dtype', ['fp16x3', 'bf16'])
def test_every_launch_q64(sncal, cuda, monkeypatch, dtype):
    """144 / 160 / 320 / 400: 2 x 64 + 16, 2 x 64 + 32, five full blocks, 6 x 64 + 16; 9 / 10 / 20 / 25 input stages."""
    stats, kinds = _run(sncal, cuda, monkeypatch, 'Q64', dtype)
    assert sorted(kinds) == ['144', '160', '320', '400'], kinds


@pytest.mark.parametrize('small_items,tile96', [('2', '4x32x96'), ('0', '8x32x96')])
def test_every_launch_m96_split_engine(sncal, cuda, monkeypatch, small_items, tile96):
    """96 / 288 / 480 / 576 on the split engine: 1, 3 and 5 blocks of 96 (6, 18 and 30 input stages), 576 refused.  Three small frames are a
    SMALL launch (hrnet_schedule.cpp tt_cfg: a few dozen items against 2 x 2 x the CU count): the 96 x 4 x 32 tile under the default
    SNCAL_TT_SMALL_ITEMS = 2, the 96 x 8 x 32 tile of the large batches with 0 -- told apart by the schedule's label."""
    stats, kinds = _run(sncal, cuda, monkeypatch, 'M96', 'fp16x3', small_items=small_items, tile96=tile96)
    assert all(k.startswith('conv<') for k in kinds['576']), kinds


def _tt_launches(widths, eligible):
    """hrnet_schedule.cpp plan_group / build_schedule, restated for members that are all two-team convolutions of one engine: the remaining
    members of a group share a launch when there are 2 or 3 of them, all eligible, and their widths padded to 96 sum to at most 744;
    otherwise the first runs alone and the rest are tried again."""
    out, i = [], 0
    while i < len(widths):
        rest = widths[i:]
        if 2 <= len(rest) <= 3 and all(eligible[i:]) and sum((w + 95) // 96 * 96 for w in rest) <= wc.TT_GROUP_MAX:
            out.append(list(rest))
            break
        out.append([rest[0]])
        i += 1
    return out


def test_every_launch_m96_bf16_and_the_group_that_must_split(sncal, cuda, monkeypatch):
    """bf16: 96 / 288 / 480 on the two-team kernel (1, 3, 5 blocks of 96), 576 on the generic one.  The launch groups hold the same-depth
    convolutions of branches 1 .. n - 1 (hrnet_graph.cpp; branch 0 is never a member, so the 864 channels of 96 + 288 + 480 never meet in one
    group).  Stage 3's group 288 + 480 = 768 > 744 (TT_COUT_MAX) must not share a launch; stage 4's 288 + 480 + 576 has a member the
    two-team kernel refuses.  In both the first member runs alone and the rest are tried again, and no eligible member may end up in a
    grouped launch of the GENERIC kernel instead (plan_group did that before this test existed: 288 and 480 on conv<bf16,...,MI6,G4>)."""
    stats, kinds = _run(sncal, cuda, monkeypatch, 'M96', 'bf16')
    c = stats['_case']
    k = 'conv_tt<bf16,k3,s1,8x32x96>'
    assert kinds['96'] == kinds['288'] == kinds['480'] == [k] and all(x.startswith('conv<bf16') for x in kinds['576']), kinds
    tt = [e for e in c['served'] if e['kernel'] == k and '.stage' in e['name']]
    w = wc.WIDTHS['M96']
    expect = 0
    for stage in (2, 3, 4):
        ok = [x % 96 == 0 and x <= wc.TT_MAX_COUT for x in w[:stage]]
        groups = [[w[0]]] + _tt_launches(list(w[1:stage]), ok[1:])           # branch 0 on its own, then the group of the other branches
        want = [g for g in ([x for x in g if x <= wc.TT_MAX_COUT] for g in groups) if g]
        assert all(len(g) == 1 for g in want), want                        # (restated rule: nothing of M96 fits one two-team launch)
        for conv in ('conv1', 'conv2'):
            level = [e for e in tt if e['name'].startswith(f'model.stage{stage}.') and e['name'].endswith(conv)]
            assert sorted(e['cout'] for e in level) == sorted(x for x in w[:stage] if x <= wc.TT_MAX_COUT), (stage, conv, level)
            got = {}
            for e in level:
                got.setdefault(e['launch'], []).append(e['cout'])
            assert sorted(sorted(v) for v in got.values()) == sorted(sorted(g) for g in want), (stage, conv, got, want)
            assert all(e['members'] == 1 for e in level), (stage, conv, level)         # 288 + 480 did not go out as one launch
            expect += len(want)
    assert expect == 2 * (2 + 3 + 3)
    # the profile row's launch count is the schedule's: one launch per convolution (+ the two-team launches outside the stages)
    outside = len({e['launch'] for e in c['served'] if e['kernel'] == k and '.stage' not in e['name']})
    assert c['profile_launches'][k] == expect + outside, (c['profile_launches'], expect, outside)


@pytest.mark.parametrize('layers', ['all', 'c288'])
def test_every_launch_m96_fp8(sncal, cuda, monkeypatch, layers):
    """e4m3 arithmetic at 96 / 288 / 480: stage counts ceil(cin / 64) = 2, 5 and 8, the last stage of 288 and 480 half empty; 3 and 5 blocks
    of 96.  'c288': only the 288-channel layers in e4m3, their neighbours in the launch groups stay bf16 (mixed members never share)."""
    stats, kinds = _run(sncal, cuda, monkeypatch, 'M96', 'fp8', fp8_layers=layers)
    k8, kb = 'conv_tt<fp8,k3,s1,8x32x96>', 'conv_tt<bf16,k3,s1,8x32x96>'
    assert kinds['288'] == [k8] and kinds['96'] == kinds['480'] == [k8 if layers == 'all' else kb], kinds
    assert all(x.startswith('conv<bf16') for x in kinds['576']), kinds
    assert stats[k8]['ops'] + stats.get(k8 + ' e4m3 out', {'ops': 0})['ops'] >= (16 if layers == 'all' else 6)       # 2 x (2 + 3 + 3) | 2 x 3 layers
    _twin_rows(stats, 'quantize_fp8 in front')


@pytest.mark.parametrize('name,dtype', [('W64', 'fp16x3'), ('P64', 'fp16x3'), ('Q64', 'fp16x3'), ('M96', 'bf16')])
def test_every_launch_one_frame_64x96(sncal, cuda, monkeypatch, name, dtype):
    """One frame of 64x96 (maps 16x24 / 8x12 / 4x6 / 2x3): no stacked-frame boundary, a single partial tile per launch on the narrow maps."""
    _run(sncal, cuda, monkeypatch, name, dtype, frames=(1, 64, 96), seed=32)
