// rm_scene_file.cpp -- see rm_scene_file.h.
#include "rm_scene_file.h"

#include <fstream>
#include <iterator>

namespace rmscene {

// ShaderLoader::preprocess (source/shader_loader.cpp:22-81): read the file
// line by line; a line holding "#include" not preceded by "//" pulls in the
// file named between "" or <> (path relative to the process CWD, no include
// guards).  Returns false with the reference's message on a missing file.
bool preprocess(const std::string &file, std::string &out, std::string &err, int depth) {
    if (depth > 64) {
        err = "ShaderLoader: #include nesting too deep at \"" + file + "\"";
        return false;
    }
    std::ifstream f(file);
    if (!f.is_open()) {
        err = "ShaderLoader: can't load file \"" + file + "\"";
        return false;
    }
    std::string line;
    while (std::getline(f, line)) {
        // text-mode reading as on the reference's platform (MSVC's fstream
        // turns CRLF into LF): without it the '\r' after a closing quote would
        // join the include name, since the name loop below re-opens on it
        if (!line.empty() && line.back() == '\r') line.pop_back();
        size_t found = line.find("#include");
        if (found != std::string::npos && (found == 0 || line.rfind("//", found) == std::string::npos)) {
            std::string name;
            bool reading = false;
            for (size_t i = found + 8; i < line.size(); i++) {
                char ch = line[i];
                if (ch == '"' || ch == '<') reading = true;
                else if (reading) {
                    if (ch == '"' || ch == '>') reading = false;
                    else name += ch;
                }
            }
            if (!preprocess(name, out, err, depth + 1)) return false;
            continue;
        }
        out += line + '\n';
    }
    return true;
}

std::string base_name(const std::string &p) {
    size_t k = p.find_last_of("/\\");
    return k == std::string::npos ? p : p.substr(k + 1);
}

int scene_of(const std::string &name) {
    if (name == "output_shader.frag" || name == "O") return kSceneO;
    if (name == "template.frag" || name == "T") return kSceneT;
    if (name == "sphere" || name == "sphere.frag" || name == "S0") return kSceneS0;
    if (name == "output_shader_glass" || name == "output_shader_glass.frag" || name == "OG") return kSceneOG;
    return -1;
}

bool is_plugin_source(const std::string &file) {
    return file.size() > 4 && file.compare(file.size() - 4, 4, ".hip") == 0;
}

// ---- scene files of registered names (the reference's "Reload scene shader",
// main.cpp:134-139, recompiles the edited output_shader.frag).  The text is
// classified by whitespace-insensitive FNV-1a 64 fingerprints of the
// reference's files (tools/ref_hashes.py; no reference text is kept):
//   output_shader.frag = prelude (up to the common.frag include) + scene part
//   (materials, floorMat, sceneSDF) + pipeline (hashes, light, render, main).
//   Reference prelude/pipeline and library: the scene part is the reference's
//   -> compiled-in scene O; an edited scene part -> compiled with hiprtc as a
//   scene plugin into output_shader.frag's pipeline.  An edited pipeline or
//   common.frag -> RM_ERR_SCENE (only the scene is re-definable).
//   template.frag: the reference's text -> scene T (repaired),
//   anything else -> RM_ERR_SCENE.
constexpr uint64_t kRefCommon = 0xac76e617a4f8cf8fULL;
constexpr uint64_t kRefTemplate = 0x39cf0bb021dfa9b7ULL;
constexpr uint64_t kRefOScene = 0x0b0b0c101eafdcf6ULL;
constexpr uint64_t kRefOFrame = 0x9ebf2dc8811b1dc0ULL;

uint64_t fingerprint(const std::string &t, uint64_t h) {
    for (unsigned char c : t) {
        if (c == ' ' || c == '\t' || c == '\r' || c == '\n' || c == '\v' || c == '\f') continue;
        h ^= c;
        h *= 0x100000001b3ULL;
    }
    return h;
}

bool read_file(const std::string &f, std::string &out) {
    std::ifstream in(f, std::ios::binary);
    if (!in.is_open()) return false;
    out.assign(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
    return true;
}

// prelude / scene / pipeline of an output_shader.frag-shaped text
// (tools/ref_hashes.py split_scene); include_name = the first #include's file
bool split_scene(const std::string &t, std::string &prelude, std::string &scene, std::string &pipeline,
                 std::string &include_name) {
    size_t k = t.find("#include");
    if (k == std::string::npos) return false;
    size_t e = t.find('\n', k);
    e = e == std::string::npos ? t.size() : e + 1;
    size_t a = t.find_first_of("\"<", k), b = a == std::string::npos ? a : t.find_first_of("\">", a + 1);
    if (a == std::string::npos || b == std::string::npos || b > e) return false;
    include_name = t.substr(a + 1, b - a - 1);
    size_t s = t.find("sceneSDF(", e);
    s = s == std::string::npos ? s : t.find('{', s);
    if (s == std::string::npos) return false;
    int depth = 0;
    for (size_t i = s; i < t.size(); i++) {
        if (t[i] == '{') depth++;
        else if (t[i] == '}' && --depth == 0) {
            prelude = t.substr(0, e);
            scene = t.substr(e, i + 1 - e);
            pipeline = t.substr(i + 1);
            return true;
        }
    }
    return false;
}

// Which scene an existing file loads as (see "scene files of registered
// names" above).  In: sc = the scene of the base name (-1 if none).  Out: sc
// (kScenePlugin: compile `src`), src = the plugin source to compile.
rm_status classify_scene_file(const std::string &file, int &sc, std::string &src, std::string &err) {
    if (sc < 0) {
        if (!is_plugin_source(file)) {
            err = "no HIP scene plugin for \"" + file + "\"";
            return RM_ERR_SCENE;
        }
        sc = kScenePlugin;
        return RM_OK;
    }
    std::string raw;
    if (!read_file(file, raw)) {
        err = "ShaderLoader: can't load file \"" + file + "\"";
        return RM_ERR_FILE;
    }
    if (sc == kSceneT) {
        if (fingerprint(raw) == kRefTemplate) return RM_OK;
        err = "\"" + file + "\" is not the reference's template.frag (which only compiles in its repaired "
              "form, scene T); write a new scene as a .hip plugin";
        return RM_ERR_SCENE;
    }
    if (sc != kSceneO) return RM_OK;  // the build's own scene names (S0, OG): no reference text
    std::string prelude, scene, pipeline, inc, lib;
    if (!split_scene(raw, prelude, scene, pipeline, inc) || fingerprint(pipeline, fingerprint(prelude)) != kRefOFrame) {
        err = "\"" + file + "\": only the scene part of output_shader.frag (materials, floorMat, sceneSDF) can "
              "be redefined; its lighting/render/main code differs from the reference's";
        return RM_ERR_SCENE;
    }
    if (!read_file(inc, lib) || fingerprint(lib) != kRefCommon) {
        err = "\"" + inc + "\" (included by \"" + file + "\") differs from the reference's common.frag: the "
              "scene library cannot be redefined; put new helpers in the scene part";
        return RM_ERR_SCENE;
    }
    if (fingerprint(scene) == kRefOScene) return RM_OK;  // the reference's own scene: compiled-in O
    sc = kScenePlugin;  // an edited sceneSDF: hiprtc into output_shader.frag's pipeline
    src = scene;
    return RM_OK;
}

rm_status load_scene_file(const std::string &file, int &sc, std::string &src, std::string &err) {
    sc = scene_of(base_name(file));
    if (!preprocess(file, src, err)) return RM_ERR_FILE;
    return classify_scene_file(file, sc, src, err);
}

}  // namespace rmscene
