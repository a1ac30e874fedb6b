// rm_plugin_batch_pack.h -- the uniform blocks of a plugin view batch
// (include/rm.h rm_render_batch_ex): from the table of what the
// loaded scene declares, the context's current block and the caller's list of
// per-view uniforms, one block per view -- the current block with view v's
// values of every listed uniform put in, as the matching rm_set_uniform* call
// would put them.  The checks of the list are here too.  Plain C++ on the host,
// no HIP: tests/host/plugin_batch_pack_test.cpp links this header with
// rm_uniform_decl.cpp alone.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/rm.h"
#include "rm_uniform_decl.h"

namespace rmpack {

// words of one view's block: the scene's slots, 16 bytes each (a scene without uniforms: 0)
inline size_t block_words(const rmuniform::Table& table) { return 4 * (size_t)table.slots; }

// What is wrong with the list, or "" if nothing is: a negative length or a list
// that is not there, then per entry, in the list's order, a NULL name or NULL
// values (n > 0), a name of the pass, an undeclared name, a name listed before,
// components that are not the declared type's, a count the declaration does not
// allow.  No value is read.
inline std::string check_view_uniforms(const rmuniform::Table& table, const rm_view_uniform* uniforms, int n_uniforms,
                                       int n) {
    if (n_uniforms < 0) return "view uniforms: n_uniforms < 0";
    if (n_uniforms > 0 && !uniforms) return "view uniforms: a null list with n_uniforms > 0";
    for (int k = 0; k < n_uniforms; k++) {
        const rm_view_uniform& u = uniforms[k];
        if (!u.name) return "view uniform " + std::to_string(k) + ": null name";
        const std::string name(u.name);
        const std::string q = "uniform \"" + name + "\"";
        if (n > 0 && !u.values) return "view " + q + ": null values";
        if (rmuniform::is_pass_name(name)) return q + " is the pass's own: a view sets u_pos, u_mouse and u_time itself";
        const rmuniform::Decl* d = table.find(name);
        if (!d) return "the loaded scene declares no " + q;
        for (int j = 0; j < k; j++)
            if (uniforms[j].name && name == uniforms[j].name) return "view " + q + " is listed twice";
        if (u.components != d->components)
            return q + " is declared " + rmuniform::type_name(*d) + ", got " + std::to_string(u.components) +
                   (u.components == 1 ? " component" : " components");
        if (u.count < 1) return "view " + q + ": count " + std::to_string(u.count) + " < 1";
        if (!d->count && u.count > 1)
            return q + " is declared " + rmuniform::type_name(*d) + ", not an array: count " + std::to_string(u.count);
        if (d->count && u.count > d->count)
            return q + " is declared " + rmuniform::type_name(*d) + ": count " + std::to_string(u.count) +
                   " is above its length";
    }
    return "";
}

// n blocks of block_words(table) words into `blocks`, view-major; `current`: the
// context's block (at least that many words).  Returns check_view_uniforms'
// message, with `blocks` left empty, if the list is refused.  An entry's values
// are n * count * components 4-byte words, view-major: floats copied as they
// are, an int as it is, a bool as 0 or 1 (non-zero: true) -- what
// rm_set_uniform{1..4}f, rm_set_uniformfv and rm_set_uniform1i store.  The words
// of a slot beyond its components, the elements of an array beyond `count` and
// every unlisted slot keep the current block's.
inline std::string pack_view_uniforms(const rmuniform::Table& table, const uint32_t* current,
                                      const rm_view_uniform* uniforms, int n_uniforms, int n,
                                      std::vector<uint32_t>& blocks) {
    blocks.clear();
    const std::string err = check_view_uniforms(table, uniforms, n_uniforms, n);
    if (!err.empty()) return err;
    const size_t words = block_words(table);
    if (n <= 0 || words == 0) return "";
    blocks.resize((size_t)n * words);
    for (int v = 0; v < n; v++) std::memcpy(blocks.data() + (size_t)v * words, current, words * sizeof(uint32_t));
    for (int k = 0; k < n_uniforms; k++) {
        const rm_view_uniform& u = uniforms[k];
        const rmuniform::Decl& d = *table.find(u.name);
        const char* src = static_cast<const char*>(u.values);
        const size_t per_view = (size_t)u.count * (size_t)u.components;
        for (int v = 0; v < n; v++) {
            uint32_t* block = blocks.data() + (size_t)v * words;
            for (int e = 0; e < u.count; e++)
                for (int c = 0; c < u.components; c++) {
                    uint32_t w;  // (memcpy: `values` need not be aligned for a word)
                    std::memcpy(&w, src + sizeof(w) * ((size_t)v * per_view + (size_t)e * u.components + c), sizeof(w));
                    if (d.type == rmuniform::kBool) w = w != 0 ? 1u : 0u;
                    block[4 * (size_t)(d.slot + e) + c] = w;
                }
        }
    }
    return "";
}

}  // namespace rmpack
