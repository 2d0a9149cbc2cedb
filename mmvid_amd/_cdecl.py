"""Strict reader of the C declarations of include/mmvid_hip.h: the prototypes, structs and constants the ctypes binding (_lib.py)
is built from, so that the header is the one place the ABI is written down.

It knows exactly the forms that header uses -- `T name(params);`, `typedef struct { fields } name_t;`, an anonymous `enum`,
`#define NAME integer` -- and refuses everything else: an unknown type, an unknown declarator, or any text left over once the forms
it knows are taken out raises CDeclError with that text.  It never skips what it does not understand.
"""
import ctypes
import os
import re
from collections import namedtuple

HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'mmvid_hip.h')
# entry points added after the list of mmvid_hip.h was pinned (tests/test_cdecl_host.py): same forms, same reader
EXT_HEADER_PATH = os.path.join(os.path.dirname(HEADER_PATH), 'mmvid_hip_ext.h')

SCALARS = {'int': ctypes.c_int, 'int32_t': ctypes.c_int, 'int64_t': ctypes.c_int64, 'uint64_t': ctypes.c_uint64,
           'float': ctypes.c_float, 'double': ctypes.c_double}
POINTEES = set(SCALARS) | {'void', 'char', 'uint8_t', 'uint16_t'}  # (the last four occur behind a pointer only)

# functions: name -> (restype, [argtypes]); structs: typedef name -> Structure class (its _fields_ are the declared fields);
# constants: the integer #defines and the enumerators.  All three keep the header's order.
Header = namedtuple('Header', 'functions structs constants')

_ITEM = re.compile(r'typedef\s+struct\s*\{(?P<fields>[^{}]*)\}\s*(?P<struct>\w+)\s*;'
                   r'|enum\s*\{(?P<enum>[^{}]*)\}\s*;'
                   r'|(?P<head>[\w\s*]+?)\((?P<params>[^(){};]*)\)\s*;')
_DECLARATOR = re.compile(r'((?:\*\s*(?:const\s*)?)*)(\w+)\s*(?:\[\s*(\d+)\s*\])?')


class CDeclError(ValueError):
    pass


def _declaration(text, structs):
    """`[const] T declarator {, declarator}` -> [(name, ctype)], declarator = `{* [const]} name [\\[N\\]]`."""
    m = re.fullmatch(r'\s*(?:const\s+)?(\w+)\b(.*)', text, re.S)
    if not m:
        raise CDeclError(f'unknown declaration: {text.strip()!r}')
    base, out = m.group(1), []
    if base not in POINTEES and base not in structs:
        raise CDeclError(f'unknown type {base!r} in {text.strip()!r}')
    for d in m.group(2).split(','):
        dm = _DECLARATOR.fullmatch(d.strip())
        if not dm:
            raise CDeclError(f'unknown declarator {d.strip()!r} in {text.strip()!r}')
        depth = dm.group(1).count('*')
        if depth == 0:
            if base not in SCALARS:
                raise CDeclError(f'type {base!r} by value in {text.strip()!r}')
            ctype = SCALARS[base]
        elif depth == 1 and base in structs:
            ctype = ctypes.POINTER(structs[base])
        elif depth == 1 and base == 'char':
            ctype = ctypes.c_char_p
        else:
            ctype = ctypes.c_void_p
        out.append((dm.group(2), ctype * int(dm.group(3)) if dm.group(3) else ctype))
    return out


def _one(text, structs):
    decls = _declaration(text, structs)
    if len(decls) != 1:
        raise CDeclError(f'one declarator expected: {text.strip()!r}')
    return decls[0]


def parse(text, class_names=None):
    """Header text -> Header.  class_names: typedef name -> name of the Structure class made for it (default: the typedef name)."""
    functions, structs, constants = {}, {}, {}

    def add(table, name, value):
        if name in functions or name in structs or name in constants:
            raise CDeclError(f'{name!r} is declared twice')
        table[name] = value

    text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
    for line in re.findall(r'^[ \t]*#.*$', text, re.M):
        if line.endswith('\\'):
            raise CDeclError(f'preprocessor line with a continuation: {line!r}')
        m = re.fullmatch(r'\s*#\s*define\s+(\w+)\s+(-?\d+)\s*', line)
        if m:
            add(constants, m.group(1), int(m.group(2)))
    text = re.sub(r'^[ \t]*#.*$', ' ', text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{(.*)\}', r'\1', text, count=1, flags=re.S)

    for m in _ITEM.finditer(text):
        try:
            if m.group('struct'):
                fields = [f for d in m.group('fields').split(';') if d.strip() for f in _declaration(d, structs)]
                name = m.group('struct')
                add(structs, name, type((class_names or {}).get(name, name), (ctypes.Structure,),
                                        {'_fields_': fields, '__doc__': f'{name} (include/mmvid_hip.h).'}))
            elif m.group('enum') is not None:
                for e in m.group('enum').split(','):
                    em = re.fullmatch(r'\s*(\w+)\s*=\s*(-?\d+)\s*', e)
                    if not em:
                        raise CDeclError(f'unknown enumerator: {e.strip()!r}')
                    add(constants, em.group(1), int(em.group(2)))
            else:
                name, restype = _one(m.group('head'), structs)
                params = m.group('params')
                args = [] if params.strip() == 'void' else [_one(p, structs)[1] for p in params.split(',')]
                add(functions, name, (restype, args))
        except CDeclError as e:
            raise CDeclError(f"{e} -- in {' '.join(m.group(0).split())[:160]!r}") from None
    rest = _ITEM.sub(' ', text).strip()
    if rest:
        raise CDeclError(f'text that is no declaration this reader knows: {rest[:200]!r}')
    return Header(functions, structs, constants)
