// rm_uniform_decl.cpp -- see rm_uniform_decl.h.
#include "rm_uniform_decl.h"

#include <cctype>
#include <cerrno>
#include <cstdlib>
#include <cstring>

namespace rmuniform {

namespace {

bool is_id(char c) { return std::isalnum((unsigned char)c) || c == '_'; }
bool is_id_start(char c) { return std::isalpha((unsigned char)c) || c == '_'; }

// the pass's own uniforms (common.frag:4-11; rm_plugin.h, rm_set_uniform*)
const char* const kPassNames[] = {"u_resolution", "u_pos",   "u_mouse", "u_time",
                                  "u_sample",     "u_sample_part", "u_seed1", "u_seed2"};

struct TypeName {
    const char* name;
    int type, components;
};
const TypeName kTypes[] = {{"float", kFloat, 1}, {"vec2", kFloat, 2}, {"vec3", kFloat, 3},
                           {"vec4", kFloat, 4},  {"int", kInt, 1},    {"bool", kBool, 1}};

// tokens of one declaration (the text between `uniform` and its ';'):
// identifiers, preprocessing numbers, single punctuation characters
std::vector<std::string> tokens(const std::string& s) {
    std::vector<std::string> t;
    size_t i = 0;
    const size_t n = s.size();
    while (i < n) {
        const char c = s[i];
        if (std::isspace((unsigned char)c)) {
            i++;
        } else if (is_id_start(c)) {
            size_t j = i;
            while (j < n && is_id(s[j])) j++;
            t.push_back(s.substr(i, j - i));
            i = j;
        } else if (std::isdigit((unsigned char)c) || (c == '.' && i + 1 < n && std::isdigit((unsigned char)s[i + 1]))) {
            size_t j = i + 1;
            while (j < n && (is_id(s[j]) || s[j] == '.' ||
                             ((s[j] == '+' || s[j] == '-') && (s[j - 1] == 'e' || s[j - 1] == 'E'))))
                j++;
            t.push_back(s.substr(i, j - i));
            i = j;
        } else {
            t.push_back(std::string(1, c));
            i++;
        }
    }
    return t;
}

uint32_t float_bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

// [sign] number at t[k...]: the float it denotes (GLSL 1.30 literals, an
// optional f suffix); k moves past it
bool float_literal(const std::vector<std::string>& t, size_t& k, float& out) {
    size_t i = k;
    bool neg = false;
    if (i < t.size() && (t[i] == "-" || t[i] == "+")) neg = t[i++] == "-";
    if (i >= t.size()) return false;
    std::string num = t[i];
    if (num.empty() || !(std::isdigit((unsigned char)num[0]) || num[0] == '.')) return false;
    const bool hex = num.size() > 1 && num[0] == '0' && (num[1] == 'x' || num[1] == 'X');
    if (!hex && (num.back() == 'f' || num.back() == 'F')) num.pop_back();
    if (num.empty()) return false;
    errno = 0;
    char* end = nullptr;
    float v;
    if (hex || num.find_first_of(".eE") == std::string::npos) {  // an integer literal converts
        const long long q = std::strtoll(num.c_str(), &end, 0);
        if (errno == ERANGE) return false;
        v = (float)q;
    } else {
        v = std::strtof(num.c_str(), &end);
        if (!(v <= 3.402823466e38f)) return false;  // out of float's range
    }
    if (!end || *end != '\0') return false;
    out = neg ? -v : v;
    k = i + 1;
    return true;
}

bool int_literal(const std::vector<std::string>& t, size_t& k, int32_t& out) {
    size_t i = k;
    bool neg = false;
    if (i < t.size() && (t[i] == "-" || t[i] == "+")) neg = t[i++] == "-";
    if (i >= t.size() || t[i].empty() || !std::isdigit((unsigned char)t[i][0])) return false;
    errno = 0;
    char* end = nullptr;
    const long long q = std::strtoll(t[i].c_str(), &end, 0);
    if (errno == ERANGE || !end || *end != '\0') return false;
    const long long v = neg ? -q : q;
    if (v < INT32_MIN || v > INT32_MAX) return false;
    out = (int32_t)v;
    k = i + 1;
    return true;
}

// the words of one declaration's text; "" or what is wrong with it
std::string parse_decl(const std::string& text, Decl& d) {
    const std::vector<std::string> t = tokens(text);
    if (t.size() < 2 || !is_id_start(t[0][0]) || !is_id_start(t[1][0]))
        return "expected `uniform <type> <name>;`";
    const TypeName* ty = nullptr;
    for (const TypeName& x : kTypes)
        if (t[0] == x.name) ty = &x;
    if (!ty)
        return "uniform type `" + t[0].substr(0, 64) + "` is not supported (float, vec2, vec3, vec4, int, bool)";
    d.type = ty->type;
    d.components = ty->components;
    d.name = t[1];
    if (d.name.size() > (size_t)kMaxName)
        return "uniform name of " + std::to_string(d.name.size()) + " characters (at most " +
               std::to_string(kMaxName) + ")";
    for (const char* p : kPassNames)
        if (d.name == p) return "`" + d.name + "` is a uniform of the pass, which provides it";
    size_t k = 2;
    if (k == t.size()) return "";
    if (t[k] == ",") return "one name per uniform declaration";
    if (t[k] == "[") {
        if (k + 2 >= t.size() || t[k + 2] != "]") return "expected `[N]` with N a decimal literal";
        const std::string& num = t[k + 1];
        long n = 0;
        for (char c : num) {
            if (!std::isdigit((unsigned char)c)) return "expected `[N]` with N a decimal literal";
            n = n > kMaxArray ? n : n * 10 + (c - '0');  // (saturates: any length of digits)
        }
        if (n < 1 || n > kMaxArray) return "array length must be 1.." + std::to_string(kMaxArray);
        if (d.type != kFloat) return "arrays of int or bool are not supported";
        d.count = (int)n;
        k += 3;
        if (k == t.size()) return "";
        return t[k] == "=" ? "an array uniform takes no initialiser" : "unexpected `" + t[k].substr(0, 64) + "`";
    }
    if (t[k] != "=") return "unexpected `" + t[k].substr(0, 64) + "` (one name per uniform declaration)";
    k++;
    const std::string bad = "initialiser must be a literal, true/false or " + std::string(ty->name) + "(literals)";
    if (d.type == kBool) {
        if (k + 1 != t.size() || (t[k] != "true" && t[k] != "false")) return "bool " + bad;
        d.def[0] = t[k] == "true";
        return "";
    }
    if (d.type == kInt) {
        int32_t v;
        if (!int_literal(t, k, v) || k != t.size()) return "int " + bad;
        d.def[0] = (uint32_t)v;
        return "";
    }
    float v[4];
    if (d.components == 1) {
        if (!float_literal(t, k, v[0]) || k != t.size()) return bad;
        d.def[0] = float_bits(v[0]);
        return "";
    }
    if (k + 1 >= t.size() || t[k] != ty->name || t[k + 1] != "(") return bad;
    k += 2;
    int n = 0;
    for (;;) {
        if (n == 4 || !float_literal(t, k, v[n])) return bad;
        n++;
        if (k < t.size() && t[k] == ",") {
            k++;
            continue;
        }
        break;
    }
    if (k + 1 != t.size() || t[k] != ")") return bad;
    if (n != 1 && n != d.components)
        return std::string(ty->name) + " initialiser takes 1 or " + std::to_string(d.components) + " literals";
    for (int i = 0; i < d.components; i++) d.def[i] = float_bits(v[n == 1 ? 0 : i]);
    return "";
}

}  // namespace

const Decl* Table::find(const std::string& name) const {
    for (const Decl& d : decls)
        if (d.name == name) return &d;
    return nullptr;
}

void Table::defaults(uint32_t block[kBlockWords]) const {
    std::memset(block, 0, kBlockWords * sizeof(uint32_t));
    for (const Decl& d : decls)
        if (!d.count) std::memcpy(block + 4 * d.slot, d.def, sizeof(d.def));
}

bool is_pass_name(const std::string& name) {
    for (const char* p : kPassNames)
        if (name == p) return true;
    return false;
}

std::string type_name(const Decl& d) {
    std::string s = d.type == kInt ? "int" : d.type == kBool ? "bool"
                    : d.components == 1 ? "float" : "vec" + std::to_string(d.components);
    if (d.count) s += "[" + std::to_string(d.count) + "]";
    return s;
}

bool parse(const std::string& src, const std::string& file, Table& table, std::string& blanked, std::string& err) {
    table = Table();
    blanked = src;
    err.clear();
    const size_t n = src.size();
    size_t i = 0;
    int line = 1, braces = 0, parens = 0;
    bool line_start = true;  // only blanks so far on this line
    auto fail = [&](int at, const std::string& msg) {
        err = file + ":" + std::to_string(at) + ": error: " + msg;
        table = Table();
        blanked = src;
        return false;
    };
    while (i < n) {
        const char c = src[i];
        if (c == '\n') {
            line++;
            line_start = true;
            i++;
            continue;
        }
        if (c == ' ' || c == '\t' || c == '\r' || c == '\v' || c == '\f') {
            i++;
            continue;
        }
        if (c == '#' && line_start) {  // a preprocessor line, with its continuations
            while (i < n && src[i] != '\n') {
                if (src[i] == '\\' && i + 1 < n && src[i + 1] == '\n') {
                    line++;
                    i++;
                }
                i++;
            }
            continue;
        }
        line_start = false;
        if (c == '/' && i + 1 < n && src[i + 1] == '/') {
            while (i < n && src[i] != '\n') i++;
            continue;
        }
        if (c == '/' && i + 1 < n && src[i + 1] == '*') {
            size_t e = src.find("*/", i + 2);
            e = e == std::string::npos ? n : e + 2;
            for (; i < e; i++) line += src[i] == '\n';
            continue;
        }
        if (c == '"' || c == '\'') {
            size_t j = i + 1;
            while (j < n && src[j] != c && src[j] != '\n') j += src[j] == '\\' ? 2 : 1;
            i = j < n && src[j] == c ? j + 1 : (j < n ? j : n);
            continue;
        }
        if (is_id_start(c) || std::isdigit((unsigned char)c)) {  // a word (a number's letters included)
            size_t j = i;
            while (j < n && is_id(src[j])) j++;
            const bool decl = braces == 0 && parens == 0 && j - i == 7 && src.compare(i, 7, "uniform") == 0;
            if (!decl) {
                i = j;
                continue;
            }
            const size_t end = src.find(';', j);
            if (end == std::string::npos) return fail(line, "uniform declaration without `;`");
            Decl d;
            d.line = line;
            const std::string msg = parse_decl(src.substr(j, end - j), d);
            if (!msg.empty()) return fail(line, msg);
            if (table.find(d.name)) return fail(line, "uniform `" + d.name + "` is declared twice");
            if (table.slots + d.slots() > kMaxSlots)
                return fail(line, "more than " + std::to_string(kMaxSlots) + " uniform slots (a uniform takes one, an "
                                  "array one per element)");
            d.slot = table.slots;
            table.slots += d.slots();
            table.decls.push_back(d);
            for (size_t k = i; k <= end; k++) {
                if (src[k] == '\n') line++;
                else blanked[k] = ' ';
            }
            i = end + 1;
            continue;
        }
        if (c == '{') braces++;
        else if (c == '}') braces -= braces > 0;
        else if (c == '(') parens++;
        else if (c == ')') parens -= parens > 0;
        i++;
    }
    return true;
}

void device_text(const Table& table, std::string& defines, std::string& undefs) {
    defines.clear();
    undefs.clear();
    std::string preload;
    for (const Decl& d : table.decls) {
        const std::string at = std::to_string(16 * d.slot);
        const std::string ty = d.components == 1 ? "float" : "vec" + std::to_string(d.components);
        std::string read;
        // (vecN names the type of the instance the scene text is compiled in)
        // (braces: `(T())[i]` would read as a cast of a lambda to a function type)
        if (d.count) read = "::rm::glsl::UniformArray<" + ty + ", " + at + ", " + std::to_string(d.count) + ">{}";
        else if (d.type == kInt) read = "::rm::glsl::uniform_i(" + at + ")";
        else if (d.type == kBool) read = "::rm::glsl::uniform_i(" + at + ") != 0";
        else read = "::rm::glsl::uniform_v<" + ty + ">(" + at + ")";
        defines += "#define " + d.name + " (" + read + ")\n";
        undefs += "#undef " + d.name + "\n";
        if (!d.count) preload += " ::rm::glsl::uniform_keep<" + at + ", " + std::to_string(d.components) + ">();";
    }
    undefs += "#define RM_UNIFORM_PRELOAD()" + preload + "\n";
}

}  // namespace rmuniform
