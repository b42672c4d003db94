"""Branch-width families beyond the packaged W18 / W32 / W48 configs, as config mappings built from four widths.

sncal_hrnet_create takes any branch width that is a multiple of 16, and the width decides the kernel, the channel block, the packing and
the launch grouping of every 3x3 stride-1 convolution of stages 2-4 (conv_tt.hpp x3_shape_ok / tt_shape_ok / ttx3_block,
hrnet_schedule.cpp plan_group).  The packaged configs reach 16 .. 384 channels in three families; the families below reach the rest:

    W64   64 / 128 / 256 / 512    full 64-channel blocks; 512 is past the two-team kernel's 480: generic kernel, 512-channel stride-2 and 1x1
    P64   80 / 112 / 176 / 240    a partial last 64-block behind full ones (80 = 64 + 16), the 48-channel last block at nb = 1, 2, 3;
                                  5 / 7 / 11 / 15 input stages of 16 channels
    Q64   144 / 160 / 320 / 400   2 x 64 + 16, 2 x 64 + 32, five full blocks, 6 x 64 + 16; 9 / 10 / 20 / 25 stages
    M96   96 / 288 / 480 / 576    3 and 5 blocks of 96, the 480 limit, 576 refused; the launch group 288 + 480 = 768 channels cannot share one launch

The launch tests run them at REDUCED depth (one module per stage, one BasicBlock per branch): the kernels see the shapes of the full depth.
`expected_kernel` restates, from the predicates, which kernel must serve a 3x3 stride-1 convolution of stages 2-4 at a given width.
"""

WIDTHS = {
    'W64': (64, 128, 256, 512),
    'P64': (80, 112, 176, 240),
    'Q64': (144, 160, 320, 400),
    'M96': (96, 288, 480, 576),
}

TT_MAX_COUT = 480          # conv_tt.hpp x3_shape_ok / tt_shape_ok: cout <= 480
TT_GROUP_MAX = 744         # conv_tt.hpp TT_COUT_MAX: channels (padded to 96) one grouped two-team launch may hold


def width_config(widths, modules=(1, 1, 1), blocks=1, stage1_blocks=1):
    """Config mapping (the field names hrnet.load_config takes) of a keypoint network whose stage s runs the first s of the four `widths`:
    stem 64, one-BOTTLENECK-family stage1 of 64 planes, upscale 2, 58 classes, log-softmax head."""
    widths = [int(w) for w in widths]
    assert len(widths) == 4, widths
    cfg = dict(num_classes=58, stem_width=64, final_conv_kernel=1, internal_final_conv=0, upscale=2, head='logsoftmax', pretrain='',
               stage1=dict(num_modules=1, num_branches=1, block_type='BOTTLENECK', num_blocks=[int(stage1_blocks)], num_channels=[64]))
    for s in (2, 3, 4):
        cfg[f'stage{s}'] = dict(num_modules=int(modules[s - 2]), num_branches=s, block_type='BASIC', num_blocks=[int(blocks)] * s,
                                num_channels=widths[:s])
    return cfg


def reduced(name):
    """The launch tests' network: num_modules 1 / 1 / 1, one BasicBlock per branch."""
    return width_config(WIDTHS[name])


def reference_depth(name):
    """The depth of the reference's own families: stage1 of 4 blocks, modules 1 / 4 / 3, 4 blocks per branch."""
    return width_config(WIDTHS[name], modules=(1, 4, 3), blocks=4, stage1_blocks=4)


def expected_kernel(engine, x3_name, cin, cout, fp8=False):
    """(label prefix, launched alone) of the kernel that must serve a 3x3 stride-1 convolution cin -> cout of stages 2-4.
    engine: 'x3' (split engine), 'bf16', 'fp8' or 'fp32'; fp8: the layer is selected for e4m3 arithmetic (only then does an fp8 engine's
    eligible layer run as conv_tt<fp8, otherwise as the bf16 engine's)."""
    if engine == 'fp32':
        return 'conv<f32,k3,s1,', False
    if engine == 'x3':
        if cin % 16 == 0 and cout % 16 == 0 and cout <= TT_MAX_COUT:
            if cout % 96 == 0:
                return f'conv_tt<{x3_name},k3,s1,', False          # ... 8x32x96 or 4x32x96, asserted to end in x96 by the caller
            return f'conv_tt<{x3_name},k3,s1,12x32x64>', True
        return f'conv<{x3_name},k3,s1,', False
    if cin % 32 == 0 and cout % 96 == 0 and cout <= TT_MAX_COUT:
        return ('conv_tt<fp8,k3,s1,' if fp8 else 'conv_tt<bf16,k3,s1,'), False
    return 'conv<bf16,k3,s1,', False
