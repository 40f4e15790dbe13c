"""CPU tests of the library's C ABIs (include/exa_*.h), every header the same way: its functions are exactly its
binding table's and all exported, every prototype has as many arguments as its argtypes, the header compiles as C99 and
C++11 and a C program over it links and runs, every struct it declares is mirrored with C's size and offsets, and a
failing call of one ABI leaves the other ABIs' last_error alone."""
import ctypes
import glob
import os
import re
import shutil
import subprocess

import pytest

from exavatar_release_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, 'include')
LIB = os.path.join(ROOT, 'exavatar_release_amd', 'libexa_raster.so')

VERSION = {'exa_raster': 139, 'exa_mesh': 100, 'exa_knn': 100, 'exa_triplane': 100, 'exa_skin': 100, 'exa_mlp': 100}
MIN_FUNCTIONS = {'exa_raster': 25}
EXACT_FUNCTIONS = {'exa_knn': 5, 'exa_triplane': 5, 'exa_skin': 5}

# Extra C statements of the linked program: host-only calls whose results it prints after the function count and the
# version, and what they must print.
PROBES = {
    # 1080 x 1920: 17 x 30 = 510 cells; 20 000 Gaussians are 20 chunks: merged scans, two-cell walk, mask-ready multi-part
    # binning, two compose trips; the two-stage protocol (fused = 0) never merges
    'exa_raster': ('  uint32_t b1 = 0, b0 = 0;\n  int r1 = exa_raster_launch_paths(1080, 1920, 20000, 1, &b1);\n'
                   '  int r0 = exa_raster_launch_paths(1080, 1920, 20000, 0, &b0);\n'
                   '  printf(" %s %d %d %u %u", exa_raster_timing_name(1), r1, r0, (unsigned)b1, (unsigned)b0);\n',
                   ['preprocess_fwd', '0', '0', str((2 << 16) | 15), str((2 << 16) | 12)]),
    # vertex 0: entry 0 (face 0 corner 0); vertex 1: entries 1, 4 (ent[2] = 4); cells 2 x 3, 1 word, 2 meshes -> 48 B -> 256
    'exa_mesh': ('  ExaMeshWorkspaceSizes s;\n  int32_t faces[6] = {0, 1, 2, 2, 1, 3}, off[5], ent[6];\n'
                 '  int rc = exa_mesh_vertex_faces(4, 2, faces, off, ent);\n'
                 '  int rw = exa_mesh_workspace_sizes(2, 10, 100, 130, &s);\n'
                 '  printf(" %d %d %d %d %d %d", rc, rw, off[1], off[2], ent[2], (int)s.bin_bytes);\n',
                 ['0', '0', '1', '3', '4', '256']),
    # two chunks of partials
    'exa_skin': ('  uint64_t b = 0;\n  int rc = exa_skin_workspace_size(257, 55, &b);\n'
                 '  printf(" %d %llu", rc, (unsigned long long)b);\n', ['0', str(2 * (12 * 55 + 3) * 4)]),
}

# One call per ABI that fails its argument checks on the host, and a word of the message it leaves.
FAILING = {
    'exa_raster': (lambda lib: lib.exa_raster_workspace_sizes(0, 0, 0, 0, None), b'out is NULL'),
    'exa_mesh': (lambda lib: lib.exa_mesh_workspace_sizes(-1, 1, 1, 1, ctypes.byref(_lib.ExaMeshWorkspaceSizes())),
                 b'negative size'),
    'exa_knn': (lambda lib: lib.exa_knn_workspace_size(1, 10, 10, 0, ctypes.byref(ctypes.c_uint64())), b'K must be'),
    'exa_triplane': (lambda lib: lib.exa_triplane_forward(-1, 1, 1, 1, None, None, None, None, None, None),
                     b'negative row count'),
    'exa_skin': (lambda lib: lib.exa_skin_workspace_size(-1, 55, ctypes.byref(ctypes.c_uint64())), b'V must be'),
    'exa_mlp': (lambda lib: lib.exa_mlp_param_count(None, ctypes.byref(ctypes.c_int64())), b'net is NULL'),
}

abis = pytest.mark.parametrize('abi', _lib.ABIS, ids=[a.prefix for a in _lib.ABIS])


def _source(abi):
    """The header without its comments and preprocessor lines."""
    src = open(os.path.join(INC, abi.header)).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return re.sub(r'^\s*#.*$', '', src, flags=re.M)


def _prototypes(abi):
    """{function: number of parameters} of every function the header declares."""
    protos = {}
    for name, params in re.findall(r'\b(exa_\w+)\s*\(([^()]*)\)\s*;', _source(abi)):
        params = params.strip()
        protos[name] = 0 if params in ('', 'void') else params.count(',') + 1
    return protos


def _structs(abi):
    return re.findall(r'typedef\s+struct\s+\w*\s*\{[^}]*\}\s*(\w+)\s*;', _source(abi))


def _run_c(tmp_path, name, text, cxx_too=False):
    """Compile `text` as C99 with every warning an error (and as C++11 if asked), link it against the library, run it
    and return its output split at white space."""
    if shutil.which('gcc') is None:
        pytest.skip('no gcc')
    src = tmp_path / (name + '.c')
    src.write_text(text)
    inc = ['-I', INC]
    subprocess.run(['gcc', '-std=c99', '-Wall', '-Wextra', '-Werror', '-Wno-pedantic', '-fsyntax-only'] + inc + [str(src)],
                   check=True)
    if cxx_too and shutil.which('g++'):
        subprocess.run(['g++', '-std=c++11', '-Wall', '-Wextra', '-Werror', '-fsyntax-only', '-x', 'c++'] + inc + [str(src)],
                       check=True)
    exe = tmp_path / name
    subprocess.run(['gcc', '-std=c99'] + inc + [str(src), LIB, '-Wl,-rpath,' + os.path.dirname(LIB),
                                                 '-Wl,--allow-shlib-undefined', '-o', str(exe)], check=True)
    rocm_lib = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'lib')
    env = dict(os.environ, LD_LIBRARY_PATH=rocm_lib + ':' + os.environ.get('LD_LIBRARY_PATH', ''))
    return subprocess.run([str(exe)], check=True, capture_output=True, text=True, env=env).stdout.split()


def test_every_header_has_one_abi_record():
    headers = sorted(os.path.basename(h) for h in glob.glob(os.path.join(INC, 'exa_*.h')))
    assert headers == sorted(a.header for a in _lib.ABIS)
    assert sorted(VERSION) == sorted(a.prefix for a in _lib.ABIS)


@abis
def test_declared_functions_are_the_table_and_are_exported(abi):
    lib = _lib.load()
    names = sorted(set(re.findall(r'\b(exa_\w+)\s*\(', _source(abi))))
    assert set(names) == set(abi.signatures), 'binding and header disagree on the exported functions'
    if abi.prefix in MIN_FUNCTIONS:
        assert len(names) >= MIN_FUNCTIONS[abi.prefix]
    if abi.prefix in EXACT_FUNCTIONS:
        assert len(names) == EXACT_FUNCTIONS[abi.prefix]
    for n in names:
        assert hasattr(lib, n), n
    assert abi.version == VERSION[abi.prefix]
    assert getattr(lib, abi.prefix + '_version')() == VERSION[abi.prefix]


def test_tables_are_disjoint_and_are_everything_load_binds():
    lib = _lib.load()
    tables = [set(a.signatures) for a in _lib.ABIS]
    union = set().union(*tables)
    assert sum(len(t) for t in tables) == len(union)
    bound = {n for n, f in vars(lib).items() if n.startswith('exa_') and f.argtypes is not None}
    assert bound == union
    for a in _lib.ABIS:
        for n, (res, args) in a.signatures.items():
            assert getattr(lib, n).restype is res and list(getattr(lib, n).argtypes) == list(args), n


@abis
def test_every_prototype_has_as_many_arguments_as_its_argtypes(abi):
    protos = _prototypes(abi)
    assert set(protos) == set(abi.signatures)
    for name, n in protos.items():
        assert n == len(abi.signatures[name][1]), '%s: %d parameters in %s, %d argtypes' % (
            name, n, abi.header, len(abi.signatures[name][1]))


@abis
def test_header_compiles_as_c99_and_cxx11_and_a_program_over_it_links_and_runs(abi, tmp_path):
    """The headers are the drop-in boundary for native hosts: each has to compile as C99 and as C++11
    without torch, HIP or any other header of ours, and a C program that takes the address of every function it
    declares and holds one of each of its structs has to link against libexa_raster.so and run (no compute call: there
    is no GPU here)."""
    names = sorted(_prototypes(abi))
    probe, expected = PROBES.get(abi.prefix, ('', []))
    text = ('#include "%s"\n#include <stdio.h>\nint main(void) {\n  void* f[] = {%s};\n' % (
        abi.header, ', '.join('(void*)' + n for n in names)))
    text += ''.join('  %s v%d; (void)v%d;\n' % (s, i, i) for i, s in enumerate(_structs(abi)))
    text += '  printf("%%d %%d", (int)(sizeof f / sizeof f[0]), %s_version());\n' % abi.prefix
    text += probe + '  printf("\\n");\n  return 0;\n}\n'
    out = _run_c(tmp_path, 'host', text, cxx_too=True)
    assert out == [str(len(names)), str(VERSION[abi.prefix])] + expected


@abis
def test_mirrored_structs_match_the_c_layout(abi, tmp_path):
    assert sorted(_structs(abi)) == sorted(abi.structs), 'every struct of the header is mirrored, nothing else'
    if not abi.structs:
        return
    lines = []
    for cname, cls in abi.structs.items():
        lines.append('  printf("%%d", (int)sizeof(%s));\n' % cname)
        lines += ['  printf(" %%d", (int)offsetof(%s, %s));\n' % (cname, f[0]) for f in cls._fields_]
        lines.append('  printf("\\n");\n')
    text = '#include <stddef.h>\n#include <stdio.h>\n#include "%s"\nint main(void) {\n%s  return 0;\n}\n' % (
        abi.header, ''.join(lines))
    out = _run_c(tmp_path, 'layout', text)
    want = []
    for cls in abi.structs.values():
        want += [str(ctypes.sizeof(cls))] + [str(getattr(cls, f[0]).offset) for f in cls._fields_]
    assert out == want
    if abi is _lib.RASTER:      # LP64: 4 ints / floats, ptr, float (+pad), 2 ptrs, int (+pad), ptr, 2 ints
        s = _lib.ExaRasterSettings
        assert ctypes.sizeof(s) == 72 and s.bg.offset == 16 and s.campos.offset == 56


@abis
def test_an_argument_error_leaves_the_other_abis_last_error_alone(abi):
    lib = _lib.load()
    last = {a.prefix: getattr(lib, a.prefix + '_last_error') for a in _lib.ABIS}
    for prefix, (call, _) in FAILING.items():       # every ABI holds a message of its own
        if prefix != abi.prefix:
            assert call(lib) < 0
    before = {p: last[p]() for p in last if p != abi.prefix}
    assert all(m.startswith(p.encode() + b': ') for p, m in before.items())
    call, word = FAILING[abi.prefix]
    assert call(lib) < 0
    assert last[abi.prefix]().startswith(abi.prefix.encode() + b': ') and word in last[abi.prefix]()
    assert {p: last[p]() for p in before} == before
    with pytest.raises(RuntimeError, match=word.decode()):
        abi.check(call(lib))
