"""CPU: the SNCAL_* environment switches of libsncal.so have one owner, csrc/env.hpp, and README.md's table says what it says.

Source checks only (the accessors themselves are exercised by tools/dev/env_host_check.cpp): no unit reads the environment behind the
table's back, every row is read somewhere, the README table repeats the rows' name, default and lifetime, and the seven switches that
were deleted for want of a user stay deleted."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'soccernet-calibration-sportlight_amd')
CSRC = os.path.join(PKG, 'csrc')
OWNERS = ('env.hpp', 'api.cpp')
ROW = re.compile(r'^\s*X\(\s*(\w+),\s*"(SNCAL_\w+)",\s*(FLAG|INT|STR),\s*(\w+),\s*(PROCESS|NET|PLAN|LAUNCH),\s*"', re.M)
DELETED = tuple('SNCAL_' + s for s in ('X3_RANGE_CHECK', 'FUSE_DECODE', 'HEAD_DECODE', 'THREE_GAIN', 'FORCE_MI_S2', 'FORCE_G_S2', 'TT_TRACE_NTH'))


def _read(path):
    with open(path, encoding='utf-8', errors='replace') as f:
        return f.read()


def _csrc():
    return {f: _read(os.path.join(CSRC, f)) for f in sorted(os.listdir(CSRC)) if os.path.isfile(os.path.join(CSRC, f))}


def _registry():
    """{name: (identifier, default as README writes it, lifetime in lower case, kind)} from the table in env.hpp."""
    rows = ROW.findall(_read(os.path.join(CSRC, 'env.hpp')))
    assert len(rows) == len({r[0] for r in rows}) == len({r[1] for r in rows}) > 0
    return {name: (ident, 'unset' if kind == 'STR' else str(int(dflt.rstrip('uUlL'), 0)), life.lower(), kind) for ident, name, kind, dflt, life in rows}


def _readme_table():
    text = _read(os.path.join(ROOT, 'README.md'))
    section = text.split('\n## Environment switches\n', 1)[1].split('\n## ', 1)[0]
    table = section.split('\n\n')[1]         # the first table: the library's own switches (the second lists what Python and bench.py read)
    rows = [[c.strip() for c in line.strip().strip('|').split('|')] for line in table.splitlines()[2:]]
    assert all(len(r) == 5 for r in rows), rows
    return {r[0].strip('`'): (r[1], r[2]) for r in rows}


def test_no_getenv_outside_the_owner():
    hits = [f for f, text in _csrc().items() if f not in OWNERS and re.search(r'\bgetenv\b', text)]
    assert hits == []


def test_registry_is_the_set_of_names_in_csrc():
    reg = _registry()
    files = _csrc()
    literals = {f: set(re.findall(r'"(SNCAL_[A-Z0-9_]+)"', text)) for f, text in files.items()}
    assert set().union(*literals.values()) == set(reg)
    assert [f for f, names in literals.items() if names and f != 'env.hpp'] == []      # a site names a row by its identifier
    sites = '\n'.join(text for f, text in files.items() if f not in OWNERS)
    by_ident = {ident: kind for ident, _, _, kind in reg.values()}
    reads = re.findall(r'\benv_(flag|int|str)\(\s*(?:sncal::)?ENV_(\w+)\s*\)', sites)
    assert len(reads) == len(re.findall(r'\bENV_\w+', sites))                          # an identifier appears in a read through an accessor only
    assert [(a, i) for a, i in reads if by_ident.get(i) != a.upper()] == []            # ... the accessor of the row's kind
    assert sorted(set(by_ident) - {i for _, i in reads}) == []                         # a row no site reads is a switch that does nothing


def test_readme_table_repeats_the_registry():
    reg = {name: (dflt, life) for name, (_, dflt, life, _) in _registry().items()}
    readme = _readme_table()
    assert sorted(readme) == sorted(reg)
    assert readme == reg


def test_deleted_switches_stay_deleted():
    """Every text file under the product, tests/, tools/, include/ and README.md; left out are tools/dev/attic (parked sources, history)
    and the package's build/ (objects), and any file with a NUL byte in it (libraries, archives, byte code)."""
    skip = {os.path.join(ROOT, 'tools', 'dev', 'attic'), os.path.join(PKG, 'build')}
    hits, seen = [], 0
    for top in ('soccernet-calibration-sportlight_amd', 'tests', 'tools', 'include', 'README.md'):
        top = os.path.join(ROOT, top)
        walk = os.walk(top) if os.path.isdir(top) else [(os.path.dirname(top), [], [os.path.basename(top)])]
        for d, subdirs, names in walk:
            subdirs[:] = [s for s in subdirs if os.path.join(d, s) not in skip]
            for n in names:
                with open(os.path.join(d, n), 'rb') as f:
                    data = f.read()
                if b'\0' not in data:
                    seen += 1
                    hits += [(os.path.relpath(os.path.join(d, n), ROOT), name) for name in DELETED if name.encode() in data]
    assert seen > 100 and hits == []
