"""tests/golden/line_cameras.npz (tools/make_golden_line_cameras.py) as the dicts and arrays the line-camera tests take."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VALUES = ('H', 'f', 'R', 'pos')
FLOOR = 2.0 ** -44


def load():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'line_cameras.npz'))


def dicts(points, offsets):
    """The packed arrays back as normalised dicts {class: [{'x', 'y'}, ...]} in ANNOT_CLASSES order: a class is a key when it owns
    a point."""
    from sncal_amd.annotations import ANNOT_CLASSES
    out = []
    for off in offsets:
        out.append({name: [{'x': float(x), 'y': float(y)} for x, y in points[off[c]:off[c + 1]]]
                    for c, name in enumerate(ANNOT_CLASSES) if off[c + 1] > off[c]})
    return out


def case(g, key):
    """Set 'A' or 'B' -> dict: 'pred' (normalised dicts), 'packed', 'peaks', 'peaks_ok', 'sizes' [(W, H)], and the capture's arrays
    under their names (status, n_lines, slots, T1, T2, H, f, R, pos, match_n, match_X, match_uv, E_ref)."""
    c = {k: g[f'{key}.{k}'] for k in ('peaks', 'peaks_ok', 'status', 'n_lines', 'slots', 'T1', 'T2', 'H', 'f', 'R', 'pos', 'match_n',
                                      'match_X', 'match_uv', 'E_ref', 'noise')}
    c['packed'] = (g[f'{key}.pred.points'], g[f'{key}.pred.offsets'])
    c['pred'] = dicts(*c['packed'])
    c['sizes'] = [tuple(int(v) for v in s) for s in g[f'{key}.img_size']]
    c['B'] = len(c['pred'])
    c['scale'], c['p_threshold'] = float(g['scale']), float(g['p_threshold'])
    return c


def by_size(c, idx=None):
    """{(W, H): [frame indices]} of the frames `idx`, in their order."""
    out = {}
    for i in (range(c['B']) if idx is None else idx):
        out.setdefault(c['sizes'][i], []).append(i)
    return out


def rel(got, want):
    """The capture's measure of a difference: max |got - want| / max |want|."""
    got, want = np.asarray(got, np.float64).ravel(), np.asarray(want, np.float64).ravel()
    return float(np.max(np.abs(got - want)) / np.max(np.abs(want)))


def bound(e_ref):
    """4 x the frame's own conditioning, with a floor of 2^-44 for frames whose E_ref underflows."""
    return 4.0 * max(float(e_ref), FLOOR)


def shares(c, b, got):
    """{quantity: rel / bound} of frame b for the quantities the capture holds; got: {quantity: array}."""
    return {k: rel(got[k], c[k][b]) / bound(c['E_ref'][b]) for k in VALUES if not np.isnan(np.asarray(c[k][b])).any()}
