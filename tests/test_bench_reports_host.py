"""CPU: every report tool's write_md reproduces the committed report from the committed figures, byte for byte
(profiles/<stem>.json -> profiles/<stem>.md).  Pins the report writers against the evidence the reviews rest on."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = {'validate': 'validate_loss', 'validate_line': 'validate_line', 'loss_grad': 'loss_grad', 'augment': 'augment',
         'jpeg_reduced': 'jpeg_reduced', 'labels': 'labels', 'extremities': 'extremities', 'sweep': 'sweep'}


@pytest.mark.parametrize('tool', sorted(TOOLS))
def test_write_md_reproduces_the_committed_report(tool, tmp_path):
    spec = importlib.util.spec_from_file_location('bench_' + tool, os.path.join(ROOT, 'tools', f'bench_{tool}.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    stem = os.path.join(ROOT, 'profiles', TOOLS[tool])
    with open(stem + '.json') as f:
        rep = json.load(f)
    mod.write_md(rep, str(tmp_path / 'r.md'))
    with open(tmp_path / 'r.md', newline='') as got, open(stem + '.md', newline='') as want:
        assert got.read() == want.read()
