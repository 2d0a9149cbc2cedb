"""The declaration reader the ctypes binding is built on (mmvid_amd/_cdecl.py): every form include/mmvid_hip.h uses, on synthetic
headers; one refusal per rule, each naming the text it refuses; the real header read completely; the built library bound from it;
and the struct layouts ctypes derives compared with the ones a C compiler derives from the same header.  No GPU: nothing here
launches a kernel."""
import ctypes
import re
import subprocess
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int64, c_uint64, c_void_p

import pytest

from mmvid_amd._cdecl import HEADER_PATH, CDeclError, parse

P, I, I64, U64, F, D = c_void_p, c_int, c_int64, c_uint64, c_float, c_double


@pytest.fixture(scope='module')
def real():
    return parse(open(HEADER_PATH).read())


def fields(cls):
    return [(n, t) for n, t in cls._fields_]


# ------------------------------------------------------------------------------------------------------- the forms, synthetic
def test_prototype_over_lines_with_a_comment_inside():
    h = parse('int mmvid_f(const float* x, int64_t ld, /* rows\n of x */ int rows,\n'
              '            uint64_t seed, float eps, double d, int32_t k,\n            void* stream);\n')
    assert h.functions == {'mmvid_f': (I, [P, I64, I, U64, F, D, I, P])} and not h.structs and not h.constants


def test_void_parameter_list_and_value_returns():
    h = parse('const char* mmvid_last(void);\nint mmvid_count(void);\nint64_t mmvid_bytes(int B);\ndouble mmvid_fill(int n);')
    assert list(h.functions.items()) == [('mmvid_last', (c_char_p, [])), ('mmvid_count', (I, [])), ('mmvid_bytes', (I64, [I])),
                                         ('mmvid_fill', (D, [I]))]


def test_several_declarators_of_one_type():
    h = parse('typedef struct {\n    const float* partial; /* [blocks] */\n    float *a, *b;\n    int N, K;\n    int64_t ld, stride;\n} s_t;')
    assert fields(h.structs['s_t']) == [('partial', P), ('a', P), ('b', P), ('N', I), ('K', I), ('ld', I64), ('stride', I64)]


def test_array_fields():
    h = parse('typedef struct { int d[3]; void* out[3]; const float* w[3]; int32_t pad; } s_t;')
    assert fields(h.structs['s_t']) == [('d', I * 3), ('out', P * 3), ('w', P * 3), ('pad', I)]
    assert ctypes.sizeof(h.structs['s_t']) == 12 + 4 + 24 + 24 + 8 and h.structs['s_t'].out.offset == 16


def test_pointer_to_const_pointer_and_other_pointers():
    h = parse('int mmvid_g(float* const* p, const float* const* q, const uint8_t* m, const uint16_t* t, const char* name, int* out);')
    assert h.functions['mmvid_g'] == (I, [P, P, P, P, c_char_p, P])
    h = parse('typedef struct { float* const* list; } s_t;')
    assert fields(h.structs['s_t']) == [('list', P)]


def test_struct_used_by_pointer_in_a_later_prototype():
    h = parse('typedef struct { int B, L; float eps; } cfg_t;\nint mmvid_run(const cfg_t* cfg, cfg_t* out, int n);', {'cfg_t': 'Cfg'})
    cfg = h.structs['cfg_t']
    assert h.functions['mmvid_run'] == (I, [POINTER(cfg), POINTER(cfg), I])
    assert cfg.__name__ == 'Cfg' and issubclass(cfg, ctypes.Structure) and fields(cfg) == [('B', I), ('L', I), ('eps', F)]
    with pytest.raises(CDeclError, match='cfg_t'):  # C's rule: a type is known from its declaration on
        parse('int mmvid_run(const cfg_t* cfg);\ntypedef struct { int B; } cfg_t;')


def test_preprocessor_lines_extern_c_defines_and_enum():
    h = parse('#ifndef H\n#define H\n#include <stdint.h>\n#ifdef __cplusplus\nextern "C" {\n#endif\n#define MMVID_V 3\n'
              'enum {\n    A = 0, /* first */\n    B = 8\n};\nint mmvid_f(void);\n#ifdef __cplusplus\n}\n#endif\n#endif\n')
    assert h.constants == {'MMVID_V': 3, 'A': 0, 'B': 8} and list(h.functions) == ['mmvid_f']


# ------------------------------------------------------------------------------------------------------------ the refusals
def test_unknown_type_is_refused():
    with pytest.raises(CDeclError, match='size_t'):
        parse('int mmvid_f(size_t n);')
    with pytest.raises(CDeclError, match='unsigned'):
        parse('typedef struct { unsigned n; } s_t;')
    with pytest.raises(CDeclError, match='uint8_t'):  # known behind a pointer only
        parse('int mmvid_f(uint8_t flag);')


def test_function_pointer_parameter_is_refused():
    with pytest.raises(CDeclError, match=re.escape('void (*cb)(int)')):
        parse('int mmvid_ok(int a);\nint mmvid_f(void (*cb)(int), int n);')
    with pytest.raises(CDeclError, match=re.escape('(*cb)(int)')):
        parse('typedef struct { void (*cb)(int); } s_t;')


def test_stray_line_is_refused():
    with pytest.raises(CDeclError, match='int mmvid_global;'):
        parse('int mmvid_f(int a);\nint mmvid_global;\nint mmvid_g(int b);')
    with pytest.raises(CDeclError, match=re.escape('// a C++ comment')):
        parse('int mmvid_f(int a); // a C++ comment\n')
    with pytest.raises(CDeclError, match=re.escape('struct tagged { int a; }')):
        parse('struct tagged { int a; };')
    with pytest.raises(CDeclError, match='mmvid_f'):  # an unnamed parameter
        parse('int mmvid_f(int);')
    with pytest.raises(CDeclError, match='twice'):
        parse('int mmvid_f(int a);\nint mmvid_f(int a);')


# ------------------------------------------------------------------------------------------------------------- the real header
def test_real_header_every_function_and_struct_once(real):
    hdr = re.sub(r'/\*.*?\*/', ' ', open(HEADER_PATH).read(), flags=re.S)
    protos = re.findall(r'\b(mmvid_\w+)\s*\(', hdr)
    typedefs = re.findall(r'\}\s*(\w+)\s*;', re.sub(r'extern "C" \{|enum \{[^}]*\};', ' ', hdr))
    assert len(protos) == len(set(protos)) == 144 and list(real.functions) == protos
    assert len(typedefs) == len(set(typedefs)) == 10 and list(real.structs) == typedefs
    assert real.constants['MMVID_ABI_VERSION'] == 3 and real.constants['MMVID_VQOP_EXT_CAST'] == 8
    assert real.constants['MMVID_VQFLAG_STRIP'] == real.constants['MMVID_VQFLAG_BLOCKS64'] == 8  # two names of one bit are both kept
    assert real.functions['mmvid_vqgan_check'] == (I, [POINTER(real.structs['mmvid_vqgan_op_t']), I])
    assert real.functions['mmvid_gemm_dw_multi_fill'] == (D, [I, POINTER(real.structs['mmvid_dw_kind_t']), I])
    assert real.functions['mmvid_set_option'] == (I, [c_char_p, I]) and real.functions['mmvid_last_error'] == (c_char_p, [])
    assert [ctypes.sizeof(s) for s in real.structs.values()] == [64, 32, 80, 192, 48, 136, 120, 96, 28, 144]


def test_binding_is_the_header(real):
    from mmvid_amd import _lib
    assert set(_lib.SIGNATURES) | set(_lib.OTHER) == set(real.functions) and not set(_lib.SIGNATURES) & set(_lib.OTHER)
    for name, (res, args) in real.functions.items():
        assert (name in _lib.OTHER) == (res is not I or name in _lib.INT_VALUED), name
        got = (_lib.OTHER[name][1], _lib.OTHER[name][0]) if name in _lib.OTHER else (I, _lib.SIGNATURES[name])
        assert len(got[1]) == len(args) and got[0] is res, name
    for py, c in _lib.STRUCTS.items():
        cls = getattr(_lib, py)
        assert cls is _lib.HEADER.structs[c] and cls.__name__ == py and fields(cls) == fields(real.structs[c])
    assert _lib.ABI_VERSION == _lib.HEADER.constants['MMVID_ABI_VERSION'] == 3


def test_built_library_exports_every_declaration_with_its_argtypes(real):
    from mmvid_amd import _lib
    from mmvid_amd.build import build
    build()
    lib = _lib.load()
    assert not lib._mmvid_missing
    for name, (res, args) in real.functions.items():
        fn = getattr(lib, name)
        assert len(fn.argtypes) == len(args) and fn.restype is res, name


def test_struct_layouts_against_the_c_compiler(real, tmp_path):
    """gcc lays the ten structs out from the header itself; ctypes lays them out from what the reader made of it."""
    lines = ['#include <stddef.h>', '#include <stdio.h>', f'#include "{HEADER_PATH}"', 'int main(void) {']
    want = []
    for name, cls in real.structs.items():
        lines.append(f'    printf("{name} %zu\\n", sizeof({name}));')
        want.append(f'{name} {ctypes.sizeof(cls)}')
        for f, _ in cls._fields_:
            lines.append(f'    printf("{name}.{f} %zu %zu\\n", offsetof({name}, {f}), sizeof((({name}*)0)->{f}));')
            want.append(f'{name}.{f} {getattr(cls, f).offset} {getattr(cls, f).size}')
    lines += ['    return 0;', '}', '']
    src, exe = tmp_path / 'layout.c', tmp_path / 'layout'
    src.write_text('\n'.join(lines))
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Wextra', '-pedantic', '-Werror', str(src), '-o', str(exe)])  # (no gcc: the test fails)
    got = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(want) == 10 + sum(len(c._fields_) for c in real.structs.values()) and got == want
