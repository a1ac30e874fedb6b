// Scene O (output_shader.hip) with four of its numbers as uniforms the host
// moves between frames without a recompile:
//     rm_load_scene(ctx, "raymarching_amd/scenes/output_shader_knobs.hip");
//     rm_set_uniform4f(ctx, "u_ball", 2.5f, 2.25f, 3.5f, 0.75f);
// At the defaults below it renders output_shader.hip's frames bit for bit.
// The smooth-minimum radii stay literals: div_k (rm_sdf_lib_body.h) has its
// fast, correctly rounded forms for constant divisors only.
uniform vec4 u_ball = vec4(3.0, 2.0, 3.0, 1.0);   // the sphere: centre, radius
uniform vec4 u_box = vec4(-5.0, 4.0, 5.0, 1.0);   // the cube: centre, half edge
uniform float u_sponge_y = 3.0;                   // height of the sponge's centre
uniform float u_spin = 2.0;                       // degrees of spin per unit of u_time

const Material kMirror = Material(vec3(0.1), vec3(0.09), 64.0, 0.25, 0.0, vec3(0.0), 1.0, vec3(0.0));
const Material kBlue = Material(vec3(0.02, 0.02, 0.2), vec3(0.02, 0.02, 0.04), 32.0, 0.0, 0.0,
                                vec3(2.0, 2.0, 0.75) * 0.2, 1.52, vec3(0.0, 0.0, 100.0));

// black/white tiles whose edges are smoothed over a width that grows with
// the distance from the origin
Material checker(vec3 pos)
{
    float blur = max(10.0, pow(length(pos), 1.3));
    vec2 t = smoothstep(-0.005, 0.005, sin(pos.xz * PI) / blur);
    float tile = min(max(t.x, t.y), max(1.0 - t.x, 1.0 - t.y));
    return Material(mix(vec3(0.3), vec3(0.025), tile), vec3(0.03), 128.0, 0.0, 0.0, vec3(0.0), 1.0, vec3(0.0));
}

SdResult sceneSDF(vec3 p)
{
    vec3 q = transformR(p - vec3(0.0, u_sponge_y, 0.0), vec3(180.0, u_time * u_spin, 0.0));
    SdResult sponge = SdResult(mengersponge(q).x, kMirror);
    SdResult ball = SdResult(sphere(u_ball, p), kBlue);
    SdResult box = SdResult(cube(u_box, p), kBlue);
    SdResult ground = SdResult(plane(p), checker(p));
    SdResult shapes = sminCubic(sminCubic(ball, box, 0.5), ground, 0.5);
    return sminCubic(sponge, shapes, 0.33);
}
