"""Generator of the recording stand-in for libzerocaf_hip.so (this module holds no test; tests/test_cpp_mirror_calls.py drives it).

source(prototypes, shapes) -> C++ text that defines every function the installed headers declare.  The functions compute nothing.
Each call appends one line to the file the environment variable ZC_STANDIN_LOG names:

    <symbol> <argument>=<value> ...            in the order of the prototype

with ctx=ok|BAD|NULL for a context, a decimal number for a by-value argument (hexadecimal for a pointer taken by value), NULL or
the hexadecimal contents of the whole extent the header entitles the call to read for an input pointer, and NULL or PTR for an
output pointer.  Then every output extent is filled: word / byte `w` of row `i` of output `o` (its index among the outputs of the
prototype) of symbol number `sid` (1 + its index in the sorted symbol list) gets pattern(sid, o, i, w) below; accept masks get
1, 0, 1, ...; a created table gets an id that is never 0 and never repeats, and its size is kept for the extents that depend on
it (TAB(id)).  ZC_STANDIN_FAIL=<symbol> makes that symbol return ZC_ERR_BAD_ARG once, after its line is logged and before
anything is filled.  ZC_STANDIN_NOFILL (any value) leaves the output extents alone (ids and the context are still handed out):
for runs of a wrapper with a planted defect that would make the stand-in write more rows than the wrapper allocated.

shapes: {symbol: {pointer argument: spec}} with the specs made by the helpers below; sizes are C expressions in the by-value
arguments of the prototype.  Context pointers need no spec."""
import re

LAST_ERROR = "stand-in: injected failure"
VERSION = "stand-in 0"
FIRST_ID = 0x5001
RETURNS = {"zc_device_count": 3, "zc_ctx_device_count": 2, "zc_ctx_device": 1}         # the calls whose status is a value


def IN(size, count):
    """an input: `count` elements of `size` bytes"""
    return ("in", size, count)


def OUT(size, per, rows="n"):
    """an output: `rows` rows of `per` elements of `size` bytes"""
    return ("out", size, per, rows)


def MASK(rows="n"):
    return ("mask", rows)


def IDOUT(size):
    """the id of a created table, which keeps `size` for TAB(id)"""
    return ("idout", size)


PARTS = ("parts",)          # nparts pointers to n rows of part_len[j] bytes
VALPTR = ("valptr",)        # a pointer the call neither reads nor writes: logged as a number
CTXOUT = ("ctxout",)


def pattern(sid, o, i, w, size):
    if size == 8:
        return (sid << 44) | (o << 40) | (i << 8) | w
    if size == 4:
        return sid * 10000 + o * 1000 + i * 50 + w
    return (sid * 7 + o * 61 + i * 29 + w * 3 + 5) & 0xFF


def mask_pattern(i):
    return 1 - (i & 1)


def parse_args(text):
    """[(type text, name, is a pointer)] of a prototype's argument list"""
    text = text.strip()
    if text in ("", "void"):
        return []
    out = []
    for piece in text.split(","):
        m = re.match(r"^(.*?)([A-Za-z_][A-Za-z0-9_]*)$", piece.strip())
        out.append((m.group(1).strip(), m.group(2), "*" in m.group(1)))
    return out


PRELUDE = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include "zerocaf_hip.h"
#include "zerocaf_hip_ext.h"
struct zc_ctx { int unused; };
namespace {
zc_ctx g_ctx;
std::map<uint64_t, size_t> g_tab;
uint64_t g_next = %(first_id)dull;
size_t TAB(uint64_t id) { auto it = g_tab.find(id); return it == g_tab.end() ? 0 : it->second; }
struct Rec {
    std::string s;
    explicit Rec(const char* sym) : s(sym) {}
    void ctx(const zc_ctx* c) { s += c == &g_ctx ? " ctx=ok" : c ? " ctx=BAD" : " ctx=NULL"; }
    void val(const char* name, long long v) { s += " " + std::string(name) + "=" + std::to_string(v); }
    void valptr(const char* name, const void* p) { char b[32]; std::snprintf(b, sizeof b, "0x%%llx", (unsigned long long)(uintptr_t)p); s += " " + std::string(name) + "=" + b; }
    void in(const std::string& name, const void* p, size_t bytes)
    {
        s += " " + name + "=";
        if (!p) { s += "NULL"; return; }
        static const char* hex = "0123456789abcdef";
        const unsigned char* q = static_cast<const unsigned char*>(p);
        for (size_t i = 0; i < bytes; i++) { s += hex[q[i] >> 4]; s += hex[q[i] & 15]; }      // reads the whole extent
    }
    void out(const char* name, const void* p) { s += " " + std::string(name) + (p ? "=PTR" : "=NULL"); }
    void flush()
    {
        const char* path = std::getenv("ZC_STANDIN_LOG");
        if (!path) return;
        if (FILE* f = std::fopen(path, "a")) { std::fprintf(f, "%%s\n", s.c_str()); std::fclose(f); }
    }
};
bool fail_once(const char* sym)
{
    static bool done = false;
    const char* e = std::getenv("ZC_STANDIN_FAIL");
    if (done || !e || std::strcmp(e, sym) != 0) return false;
    done = true;
    return true;
}
bool nofill() { return std::getenv("ZC_STANDIN_NOFILL") != nullptr; }
void fill(int sid, int o, void* p, size_t size, size_t per, size_t rows)
{
    if (!p || nofill()) return;
    for (size_t i = 0; i < rows; i++)
        for (size_t w = 0; w < per; w++) {
            unsigned char* at = static_cast<unsigned char*>(p) + (i * per + w) * size;
            if (size == 8) { const uint64_t v = ((uint64_t)sid << 44) | ((uint64_t)o << 40) | ((uint64_t)i << 8) | (uint64_t)w; std::memcpy(at, &v, 8); }
            else if (size == 4) { const int32_t v = (int32_t)(sid * 10000 + o * 1000 + (int)i * 50 + (int)w); std::memcpy(at, &v, 4); }
            else *at = (unsigned char)((sid * 7 + o * 61 + (int)i * 29 + (int)w * 3 + 5) & 0xFF);
        }
}
void fill_mask(uint8_t* p, size_t rows)
{
    if (!p || nofill()) return;
    for (size_t i = 0; i < rows; i++) p[i] = (uint8_t)(1 - (i & 1));
}
}  // namespace
extern "C" {
const char* zc_last_error(void) { Rec r("zc_last_error"); r.flush(); return "%(last_error)s"; }
const char* zc_version(void) { Rec r("zc_version"); r.flush(); return "%(version)s"; }
"""


def source(prototypes, shapes):
    names = sorted(name for name, _ in prototypes)
    assert len(set(names)) == len(names)
    unknown = sorted(set(shapes) - set(names))
    assert not unknown, "shapes for symbols no header declares: %s" % unknown
    sid = {n: i + 1 for i, n in enumerate(names)}
    text = [PRELUDE % dict(first_id=FIRST_ID, last_error=LAST_ERROR, version=VERSION)]
    for name, argtext in prototypes:
        if name in ("zc_last_error", "zc_version"):
            continue
        args = parse_args(argtext)
        spec = dict(shapes.get(name, {}))
        log, after = [], []
        o = 0
        for typ, arg, is_ptr in args:
            if typ.replace("const", "").replace(" ", "") == "zc_ctx*":
                log.append("r.ctx(%s);" % arg)
                continue
            if not is_ptr:
                assert arg not in spec, (name, arg)
                log.append('r.val("%s", (long long)%s);' % (arg, arg))
                continue
            assert arg in spec, "no shape for pointer %s of %s" % (arg, name)
            s = spec.pop(arg)
            if s[0] == "in":
                log.append('r.in("%s", %s, (size_t)(%s) * %d);' % (arg, arg, s[2], s[1]))
            elif s[0] == "parts":
                log.append('for (size_t j_ = 0; j_ < nparts; j_++) r.in("%s." + std::to_string(j_), %s ? %s[j_] : nullptr, part_len[j_] * n);' % (arg, arg, arg))
            elif s[0] == "valptr":
                log.append('r.valptr("%s", %s);' % (arg, arg))
            elif s[0] == "out":
                log.append('r.out("%s", %s);' % (arg, arg))
                after.append("fill(%d, %d, %s, %d, (size_t)(%s), (size_t)(%s));" % (sid[name], o, arg, s[1], s[2], s[3]))
                o += 1
            elif s[0] == "mask":
                log.append('r.out("%s", %s);' % (arg, arg))
                after.append("fill_mask(%s, (size_t)(%s));" % (arg, s[1]))
                o += 1
            elif s[0] == "idout":
                log.append('r.out("%s", %s);' % (arg, arg))
                after.append("if (%s) { *%s = g_next; g_tab[g_next++] = (size_t)(%s); }" % (arg, arg, s[1]))
                o += 1
            elif s[0] == "ctxout":
                log.append('r.out("%s", %s);' % (arg, arg))
                after.append("if (%s) *%s = &g_ctx;" % (arg, arg))
                o += 1
            else:
                raise AssertionError(s)
        assert not spec, "shapes of %s name arguments it does not have: %s" % (name, sorted(spec))
        body = ['    Rec r("%s");' % name] + ["    " + l for l in log] + ["    r.flush();", '    if (fail_once("%s")) return ZC_ERR_BAD_ARG;' % name]
        body += ["    " + l for l in after] + ["    return %d;" % RETURNS.get(name, 0)]
        text.append("int %s(%s)\n{\n%s\n}\n" % (name, argtext if argtext.strip() else "void", "\n".join(body)))
    text.append("}  // extern \"C\"\n")
    return "".join(text)
