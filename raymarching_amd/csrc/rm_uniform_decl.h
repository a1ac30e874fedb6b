// rm_uniform_decl.h -- `uniform` declarations of a scene source (include/rm.h,
// rm_load_scene): the table of what a scene declares, and the scene text with
// the declarations blanked.  Plain C++, no HIP: tests/host/uniform_decl_test.cpp
// links rm_uniform_decl.cpp alone.
//
// At file scope (brace and parenthesis depth 0, outside comments, string
// literals and preprocessor lines) a scene may say
//     uniform <type> <name>;            type: float vec2 vec3 vec4 int bool
//     uniform <type> <name> = <init>;   a literal, true/false, or vecN(literals)
//     uniform <ftype> <name>[N];        ftype: float vec2 vec3 vec4; N = 1..64
// Matching is textual: a declaration in an inactive #if region still counts.
// The values live in a block of kMaxSlots slots of 16 bytes that the plugin's
// kernels take as an argument (rm_plugin.h): a non-array uniform owns one
// slot, an array one slot per element.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace rmuniform {

constexpr int kMaxSlots = 64;                        // 16 bytes each
constexpr int kBlockWords = kMaxSlots * 4;           // the value block, 1 KiB
constexpr int kMaxArray = 64;
constexpr int kMaxName = 63;

enum Type { kFloat = 0, kInt = 1, kBool = 2 };  // include/rm.h rm_uniform_type

struct Decl {
    std::string name;
    int type = kFloat;
    int components = 1;  // 1..4 (int and bool: 1)
    int count = 0;       // array length; 0: not an array
    int slot = 0;        // first slot
    int line = 0;        // of the `uniform` keyword, 1-based
    uint32_t def[4] = {0, 0, 0, 0};  // default words (arrays start at zero)

    int slots() const { return count ? count : 1; }
};

struct Table {
    std::vector<Decl> decls;  // declaration order
    int slots = 0;

    const Decl* find(const std::string& name) const;
    // the block a freshly loaded scene starts with: every default, zero elsewhere
    void defaults(uint32_t block[kBlockWords]) const;
};

// a uniform of the pass itself (u_time, u_pos, ...: no scene may declare one)
bool is_pass_name(const std::string& name);

// the GLSL spelling of a declaration's type ("vec4", "float[8]"), for messages
std::string type_name(const Decl& d);

// Reads the declarations of `src` into `table` and writes `blanked`: `src`
// with every declaration replaced by spaces (newlines kept, so every later
// line keeps its number).  False with "file:line: error: ..." in `err` for a
// declaration outside the dialect, a name the pass provides, a name declared
// twice, or more than kMaxSlots slots.
bool parse(const std::string& src, const std::string& file, Table& table, std::string& blanked, std::string& err);

// What the declarations turn into for the compiler (rm_plugin_host.cpp's
// translation unit): `defines`, one function-like read per name, to go before
// the scene's two instances; `undefs`, which takes the names back after them
// and defines RM_UNIFORM_PRELOAD(), the loads of every non-array uniform at
// the top of each kernel (rm_plugin_kernels.h).
void device_text(const Table& table, std::string& defines, std::string& undefs);

}  // namespace rmuniform
