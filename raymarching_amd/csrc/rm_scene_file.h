// rm_scene_file.h -- scene-file text handling of rm_load_scene / rm_compile_scene:
// the reference's ShaderLoader and the classification of a file by name and
// fingerprint.  Plain C++ (no HIP), so tests/host/host_logic_test.cpp calls it.
#pragma once
#include <cstdint>
#include <string>

#include "../../include/rm.h"

namespace rmscene {

// rm::SceneId's values (rm_device.h; rm_capi.cpp pins the two together)
constexpr int kSceneS0 = 0, kSceneT = 1, kSceneO = 2, kSceneOG = 3, kScenePlugin = 4;

bool preprocess(const std::string &file, std::string &out, std::string &err, int depth = 0);
std::string base_name(const std::string &p);
int scene_of(const std::string &name);  // the scene of a registered (base) name, or -1
bool is_plugin_source(const std::string &file);
uint64_t fingerprint(const std::string &t, uint64_t h = 0xcbf29ce484222325ULL);
bool read_file(const std::string &f, std::string &out);
bool split_scene(const std::string &t, std::string &prelude, std::string &scene, std::string &pipeline,
                 std::string &include_name);
rm_status classify_scene_file(const std::string &file, int &sc, std::string &src, std::string &err);
// An existing file as rm_load_scene and rm_compile_scene read it: the scene of
// its base name, its preprocessed text, classify_scene_file.  Out: sc, src.
rm_status load_scene_file(const std::string &file, int &sc, std::string &src, std::string &err);

}  // namespace rmscene
