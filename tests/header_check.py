"""Python's statement of the C boundary held to the headers BY THE COMPILER: the ctypes.Structure mirrors (gltf_renderer_amd/abi.py,
gltf.py) against the typedefs, and the prototype tables (abi.PROTOTYPES, gltf.SCENE_PROTOTYPES, tests/hooks.py HOOKS) against the
declarations.  Also header_text(), the one reader of a header for the tests that assert what its text says (enum and #define values,
documented defaults and sizes).  Used by tests/test_host_abi.py; CPU only, g++ only."""
import ctypes as C
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
CSRC = os.path.join(ROOT, "gltf_renderer_amd", "csrc")


def header_text(name="mipt.h", comments=True):
    """The text of include/<name> (or of csrc/<name>, for mipt_debug.h); comments=False blanks the /* ... */ comments out."""
    path = os.path.join(INCLUDE, name)
    text = open(path if os.path.exists(path) else os.path.join(CSRC, name)).read()
    return text if comments else re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def typedef_structs(name):
    """The names of every `typedef struct <name> {` of a header."""
    return re.findall(r"typedef\s+struct\s+(\w+)\s*\{", header_text(name, comments=False))


def typedef_struct(struct, name="mipt.h"):
    """(the body of `typedef struct <struct> { ... } <struct>;` with its comments, the rest of the closing line: the size the header states)."""
    m = re.search(r"typedef struct %s \{(.*?)\} %s;([^\n]*)" % (struct, struct), header_text(name), re.S)
    assert m, "include/%s lacks %s" % (name, struct)
    return m.group(1), m.group(2)


def stated_bytes(struct, name="mipt.h"):
    """The N of the `/* N bytes */` the header puts after a typedef."""
    return int(re.search(r"/\* (\d+) bytes \*/", typedef_struct(struct, name)[1]).group(1))


def declared_functions(name, pattern):
    """The names matching `pattern` that a header declares (followed by an opening parenthesis, outside comments)."""
    return sorted(set(re.findall(r"\b(%s)\s*\(" % pattern, header_text(name, comments=False))))


def c_name(cls):
    """PtAovConfig -> pt_aov_config: a mirror class's typedef."""
    return re.sub(r"(?<!^)(?=[A-Z])", "_", cls.__name__).lower()


def mirrors(module):
    """{typedef name: class} of every ctypes.Structure a module defines (an alias such as abi._TS is the class it names, once)."""
    return {c_name(c): c for n, c in vars(module).items() if inspect.isclass(c) and issubclass(c, C.Structure) and c.__module__ == module.__name__ and n == c.__name__}


def type_class(t):
    """A ctypes type's class as the compiler will be asked for it: 'p' pointer, 'f4' float, 'i4' / 'u4' / 'u8' ... integers by signedness and
    size, 'v' void (a restype of None), 'S<typedef>' a structure.  An array's class is its element's."""
    if t is None:
        return "v"
    if issubclass(t, C.Array):
        return type_class(t._type_)
    if issubclass(t, C.Structure):
        return "S" + c_name(t)
    if issubclass(t, C._Pointer) or t._type_ in "PzZ":
        return "p"
    kind = "f" if t._type_ in "fdg" else "i" if t._type_ in "bhilq" else "u" if t._type_ in "BHILQ" else None
    assert kind, "no class for %r" % t
    return "%s%d" % (kind, C.sizeof(t))


# what the generated translation units share: kind<T>() and width<T>() name T's class as type_class() names a ctypes type's
_PRELUDE = r'''
#include <cstddef>
#include <cstdio>
#include <type_traits>
#include "mipt_scene.h"
#include "mipt_debug.h"
template <typename T> struct elem { using type = T; };
template <typename T, size_t N> struct elem<T[N]> { using type = T; };
template <typename T> constexpr char kind() {
    using E = typename elem<T>::type;
    return std::is_void<E>::value ? 'v' : std::is_pointer<E>::value ? 'p' : std::is_floating_point<E>::value ? 'f'
         : std::is_integral<E>::value ? (std::is_signed<E>::value ? 'i' : 'u') : 'S';
}
template <typename T> constexpr size_t width() { using E = typename elem<T>::type; return sizeof(typename std::conditional<std::is_void<E>::value, char, E>::type); }
'''


def _compile(source, tmp_path, name, run=False):
    """Compiles `source` with g++ (syntax only unless `run`); returns (exit status, the compiler's messages, the program's output)."""
    src = os.path.join(str(tmp_path), name + ".cpp")
    open(src, "w").write(source)
    cmd = ["g++", "-std=c++17", "-I", INCLUDE, "-I", CSRC]
    exe = os.path.join(str(tmp_path), name)
    cc = subprocess.run(cmd + (["-o", exe] if run else ["-fsyntax-only"]) + [src], capture_output=True, text=True)
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout if run and cc.returncode == 0 else ""
    return cc.returncode, cc.stderr, out


def layout_source(structs):
    """One static_assert on the size of every mirror, and per field one on its offset, one on its size and one on its class."""
    lines = [_PRELUDE]
    for cname, cls in sorted(structs.items()):
        lines.append('static_assert(sizeof(%s) == %d, "sizeof %s");' % (cname, C.sizeof(cls), cname))
        for field, ftype in cls._fields_:
            d, where = getattr(cls, field), "%s.%s" % (cname, field)
            lines.append('static_assert(offsetof(%s, %s) == %d, "offset of %s");' % (cname, field, d.offset, where))
            lines.append('static_assert(sizeof(%s::%s) == %d, "size of %s");' % (cname, field, d.size, where))
            k = type_class(ftype)
            if k[0] == "S":
                lines.append('static_assert(std::is_same<elem<decltype(%s::%s)>::type, %s>::value, "type of %s");' % (cname, field, k[1:], where))
            else:
                want = "kind<decltype(%s::%s)>() == '%s'" % (cname, field, k[0]) + (" && width<decltype(%s::%s)>() == %s" % (cname, field, k[1:]) if k[1:] else "")
                lines.append('static_assert(%s, "class of %s");' % (want, where))
    return "\n".join(lines) + "\n"


def check_layouts(structs, tmp_path):
    """The compiler's messages about layout_source(structs): empty if every mirror is its typedef byte for byte and class for class."""
    rc, err, _ = _compile(layout_source(structs), tmp_path, "layout")
    return err if rc else ""


def declared_signatures(names, tmp_path):
    """{name: [class of the return type, class of each parameter ...]} as the compiler reads the declarations of `names` in the headers."""
    src = _PRELUDE + r'''
template <typename T> void put() { if (kind<T>() == 'p' || kind<T>() == 'v') std::printf(" %c", kind<T>()); else std::printf(" %c%zu", kind<T>(), width<T>()); }
template <typename F> struct sig;
template <typename R, typename... A> struct sig<R (*)(A...)> { static void print(const char* name) { std::printf("%s", name); put<R>(); (put<A>(), ...); std::printf("\n"); } };
int main() {
''' + "".join('    sig<decltype(&%s)>::print("%s");\n' % (n, n) for n in names) + "    return 0;\n}\n"
    rc, err, out = _compile(src, tmp_path, "signatures", run=True)
    assert rc == 0, err
    return {row[0]: row[1:] for row in (line.split() for line in out.splitlines())}


def table_signatures(table):
    """The same of a prototype table's rows."""
    return {name: [type_class(restype)] + [type_class(a) for a in argtypes] for name, (restype, argtypes) in table.items()}
