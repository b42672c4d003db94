#!/usr/bin/env python3
"""Did a source change alter the device code?  Compiles every csrc/*.hip of two trees to gfx950 assembly and prints, per unit, how many
lines differ.  No GPU needed.

    python tools/dev/isa_diff.py PARENT_TREE NEW_TREE [--rename OLD=NEW ...] [-DSNCAL_X3_F16=0] [--only conv_tt.hip] [--allow-reorder solve.hip] [--jobs 16] [--keep DIR]

Each tree's csrc/ and include/ are copied in turn to the SAME temporary path before they are compiled, because source paths leak into
the assembly.  The flags are build.py's CXXFLAGS (of the tree being compiled) plus --cuda-device-only -S, plus any -D given here.  Lines
that differ between any two builds are dropped: `__hip_cuid_*`, `.file`, `.ident`.  --rename replaces a symbol name of the parent's
assembly by the new tree's (mangled kernel names after a renaming refactor); where several old names map to one new name, a line that
becomes identical to the line before it is dropped (three `.addrsig_sym` lines of one LDS symbol per namespace becoming one).  For a unit
named with --allow-reorder (solve.hip: hipcc emits its two .rodata tables in either order, from one compilation of the same source to
the next) the same lines in another order count as identical, and the table says so; for every other unit moved lines differ.
The tool diffs two builds; it inspects nothing else in the assembly."""
import argparse
import collections
import difflib
import importlib.util
import os
import shutil
import subprocess
import sys
import tempfile


def package_dir(tree):
    found = [d for d in sorted(os.listdir(tree)) if os.path.isdir(os.path.join(tree, d, 'csrc'))]
    if len(found) != 1:
        sys.exit(f'{tree}: expected exactly one <package>/csrc, found {found}')
    return found[0]


def cxxflags(tree, pkg):
    spec = importlib.util.spec_from_file_location('sncal_build_' + str(abs(hash(tree))), os.path.join(tree, pkg, 'build.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return list(mod.CXXFLAGS), mod._hipcc()


def compile_tree(tree, work, out, defines, only, jobs):
    """tree's sources -> work (always the same path) -> out/<unit>.s"""
    pkg = package_dir(tree)
    flags, hipcc = cxxflags(tree, pkg)
    shutil.rmtree(work, ignore_errors=True)
    shutil.copytree(os.path.join(tree, pkg, 'csrc'), os.path.join(work, 'pkg', 'csrc'))
    shutil.copytree(os.path.join(tree, 'include'), os.path.join(work, 'include'))
    os.makedirs(out, exist_ok=True)
    csrc = os.path.join(work, 'pkg', 'csrc')
    units = sorted(f for f in os.listdir(csrc) if f.endswith('.hip') and (not only or f in only))
    running, failed = [], []

    def reap(block):
        for item in list(running):
            u, p = item
            if block or p.poll() is not None:
                text = p.communicate()[0]
                if p.returncode != 0:
                    failed.append(u)
                    sys.stderr.write(text.decode(errors='replace'))
                running.remove(item)
                if block:
                    return

    for u in units:
        while len(running) >= jobs:
            reap(False)
            if len(running) >= jobs:
                reap(True)
        cmd = [hipcc, '-x', 'hip', *flags, *defines, '--cuda-device-only', '-S', u, '-o', os.path.join(out, u[:-4] + '.s')]
        running.append((u, subprocess.Popen(cmd, cwd=csrc, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)))
    while running:
        reap(True)
    if failed:
        sys.exit(f'{tree}: hipcc failed on {failed}')
    return units


def normalised(path, renames):
    lines = []
    for line in open(path, errors='replace').read().split('\n'):
        s = line.strip()
        if '__hip_cuid_' in line or s.startswith('.file') or s.startswith('.ident'):
            continue
        renamed = line
        for old, new in renames:
            renamed = renamed.replace(old, new)
        if renamed != line and lines and lines[-1] == renamed:
            continue
        lines.append(renamed)
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('parent')
    ap.add_argument('new')
    ap.add_argument('--rename', action='append', default=[], metavar='OLD=NEW')
    ap.add_argument('-D', action='append', default=[], dest='defines', metavar='NAME=VALUE')
    ap.add_argument('--only', nargs='*', metavar='UNIT.hip')
    ap.add_argument('--allow-reorder', nargs='*', metavar='UNIT.hip',
                    help='units for which the same lines in another order count as identical (solve.hip: its two .rodata tables)')
    ap.add_argument('--jobs', type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument('--keep', metavar='DIR', help='keep the assembly files under DIR/parent and DIR/new')
    ap.add_argument('--show', type=int, default=0, metavar='N', help='print the first N differing lines of each unit')
    args = ap.parse_args()
    renames = [tuple(r.split('=', 1)) for r in args.rename]
    # longest first, so that a name that is a prefix of another one does not eat it
    renames.sort(key=lambda r: -len(r[0]))
    defines = ['-D' + d for d in args.defines]
    base = args.keep or tempfile.mkdtemp(prefix='isa_diff_out_')
    work = os.path.join(tempfile.mkdtemp(prefix='isa_diff_tree_'), 't')      # one path per run, the same for both trees
    try:
        units_a = compile_tree(os.path.abspath(args.parent), work, os.path.join(base, 'parent'), defines, args.only, min(16, args.jobs))
        units_b = compile_tree(os.path.abspath(args.new), work, os.path.join(base, 'new'), defines, args.only, min(16, args.jobs))
        total = 0
        print(f'{"unit":<20}{"parent":>9}{"new":>9}{"differing":>11}')
        for u in sorted(set(units_a) | set(units_b)):
            if u not in units_a or u not in units_b:
                print(f'{u:<20} only in the {"parent" if u in units_a else "new tree"}')
                total += 1
                continue
            a = normalised(os.path.join(base, 'parent', u[:-4] + '.s'), renames)
            b = normalised(os.path.join(base, 'new', u[:-4] + '.s'), [])
            diff = [] if a == b else [d for d in difflib.unified_diff(a, b, lineterm='', n=0) if d[:1] in '+-' and d[:3] not in ('+++', '---')]
            note = ''
            if diff and u in (args.allow_reorder or []) and collections.Counter(a) == collections.Counter(b):
                note, diff = f'  ({len(diff)} lines moved: the same lines in another order)', []
            print(f'{u:<20}{len(a):>9}{len(b):>9}{len(diff):>11}{note}')
            for d in diff[:args.show]:
                print('    ' + d[:200])
            total += len(diff)
        print(f'{total} differing lines in all' + (f' (-D {" ".join(args.defines)})' if args.defines else ''))
        return 1 if total else 0
    finally:
        shutil.rmtree(os.path.dirname(work), ignore_errors=True)
        if not args.keep:
            shutil.rmtree(base, ignore_errors=True)


if __name__ == '__main__':
    sys.exit(main())
