"""A/B helper: are two builds of libsncal.so the same function?  One run (one library: SNCAL_LIB_PATH, or tuning env vars that
are read once per process) writes, per combination of the matrix below, the sha-256 of heatmap + keypoints, of the keypoints-only
call, the workspace bytes and the profile rows of one profiled forward; a second invocation compares two such files.
    python tools/dev/ab_equal.py --out a.json [--only w48] ;  python tools/dev/ab_equal.py --compare a.json b.json"""
import argparse, hashlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

ENGINES = ('fp32', 'bf16', 'fp8', 'fp16x3')
# (name, config, H, W, batches run on ONE net, SNCAL_SUBBATCH or None, SNCAL_FUSED_HEAD, seed): full sub-batches and a shorter last one
GROUPS = [
    ('w48', 'hrnet_w48', 540, 960, (64, 67), None, 1, 1),
    ('w48_unfused', 'hrnet_w48', 540, 960, (6,), 4, 0, 1),
    ('w32', 'hrnet_w32', 270, 480, (8, 9), 4, 1, 3),
    ('w32_unfused', 'hrnet_w32', 270, 480, (5,), 4, 0, 3),
    ('w18', 'hrnet_w18', 540, 960, (8,), None, 1, 4),
    ('line_w48', 'line_hrnet_w48', 540, 960, (5,), 4, 1, 2),
]


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.cpu().numpy().tobytes())
    return h.hexdigest()[:24]


def run(out_path, only):
    import torch
    import sncal_amd
    from bench import seeded_weights
    dev = torch.device('cuda:0')
    res = {}
    for name, cfg, H, W, batches, subbatch, fused, seed in GROUPS:
        if only and name not in only:
            continue
        sd = seeded_weights(cfg, seed)
        os.environ['SNCAL_FUSED_HEAD'] = str(fused)          # both are read when the network is created
        os.environ.pop('SNCAL_SUBBATCH', None)
        if subbatch:
            os.environ['SNCAL_SUBBATCH'] = str(subbatch)
        for dtype in ENGINES:
            line = cfg.startswith('line_')                   # softmax head: no keypoint decode, so no fp8 calibration either
            if line and dtype == 'fp8':
                continue
            net = sncal_amd.HRNetHeatmap(cfg, dtype=dtype, device=dev)
            net.load_state_dict(sd)
            for B in batches:
                x = torch.rand((B, 3, H, W), device=dev, generator=torch.Generator(device=dev).manual_seed(5))
                if dtype == 'fp8':
                    net.calibrate_fp8(x[:min(B, 8)])
                r = {}
                heat, kp = net.forward(x, want_heat=True, decode_size=None if line else (H, W))
                r['heat_kp'] = sha(heat) if line else sha(heat, kp)
                if not line:
                    r['kp_only'] = sha(net.forward(x, want_heat=False, decode_size=(H, W))[1])
                r['workspace'] = int(net._workspace(B, H, W).numel())
                net.set_profiling(1)
                net.forward(x, want_heat=line, decode_size=None if line else (H, W))
                r['profile'] = sorted((p['kernel'], p['flops'], p['bytes'], p['launches']) for p in net.get_profile())
                r['labels'] = [op['kernel'] for op in net.plan_ops()]
                net.set_profiling(0)
                key = f'{name}/{dtype}/B{B}'
                res[key] = r
                print(key, r['heat_kp'], r.get('kp_only'), r['workspace'], len(r['profile']), flush=True)
                with open(out_path, 'w') as f:
                    json.dump(res, f)
            del net


def compare(a_path, b_path):
    a, b = json.load(open(a_path)), json.load(open(b_path))
    bad = [k for k in sorted(set(a) | set(b)) if a.get(k) != b.get(k)]
    for k in bad:
        fields = [f for f in ('heat_kp', 'kp_only', 'workspace', 'profile', 'labels') if (a.get(k) or {}).get(f) != (b.get(k) or {}).get(f)]
        print('DIFFERENT', k, fields)
    print(f'{len(a)} / {len(b)} combinations, {len(bad)} different')
    return 1 if bad or not a else 0


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out')
    ap.add_argument('--only', nargs='*')
    ap.add_argument('--compare', nargs=2)
    args = ap.parse_args()
    sys.exit(compare(*args.compare) if args.compare else run(args.out, args.only))
