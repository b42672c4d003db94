"""tests/golden/extremities.npz (tools/make_golden_extremities.py) as the dicts and arrays the extremity tests take."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = ('packed', 'peaks')


def load():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'extremities.npz'))


def dicts(points, offsets):
    """The packed arrays back as normalised dicts {class: [{'x', 'y'}, ...]}: a class is a key when it owns a point."""
    from sncal_amd.annotations import ANNOT_CLASSES
    out = []
    for off in offsets:
        out.append({name: [{'x': float(x), 'y': float(y)} for x, y in points[off[c]:off[c + 1]]]
                    for c, name in enumerate(ANNOT_CLASSES) if off[c + 1] > off[c]})
    return out


def case(g, key):
    """Set 'A' or 'B' -> dict of its inputs (normalised dicts, packed tuples, peaks) and expected outputs per form."""
    size = tuple(int(v) for v in g[f'{key}.img_size'])
    c = {'size': size, 'ts': tuple(float(t) for t in g[f'{key}.ts']), 'scale': float(g[f'{key}.scale']),
         'p_threshold': float(g[f'{key}.p_threshold']), 'peak_rows': g[f'{key}.peaks'],
         'gt_packed': (g[f'{key}.gt.points'], g[f'{key}.gt.offsets'], None),
         'pred_packed': (g[f'{key}.pred.points'], g[f'{key}.pred.offsets'], None)}
    c['gt'] = dicts(*c['gt_packed'][:2])
    c['pred'] = dicts(*c['pred_packed'][:2])
    c['B'] = len(c['gt'])
    for form in FORMS:
        c[form] = {k: g[f'{key}.{form}.{k}'] for k in ('frame', 'cls', 'err', 'agg', 'per_class')}
    return c


def pixels(c, form):
    """(predictions, annotations) of a case as the PIXEL dicts the host function takes, for one prediction form."""
    from sncal_amd.evaluate import scale_points
    from sncal_amd.extremities import peaks_to_points
    W, H = c['size']
    gts = [scale_points(a, W, H) for a in c['gt']]
    if form == 'packed':
        return [scale_points(a, W, H) for a in c['pred']], gts
    return [peaks_to_points(p, c['scale'], c['p_threshold']) for p in c['peak_rows']], gts


def agg_array(res):
    """aggregate()'s dict -> ((3,3) [accuracy, precision, recall] x [mean, std, median], (28,3) per-class table with NaN rows)."""
    from sncal_amd.annotations import ANNOT_CLASSES
    agg = np.array([[res[k][s] for s in ('mean', 'std', 'median')] for k in ('accuracy', 'precision', 'recall')])
    table = np.full((len(ANNOT_CLASSES), 3), np.nan)
    for name, row in res['per_class'].items():
        table[ANNOT_CLASSES.index(name)] = (row['accuracy'], row['precision'], row['recall'])
    return agg, table


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)
