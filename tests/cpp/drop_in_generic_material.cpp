// tests/cpp/drop_in_generic_material.cpp -- a generic_material application on the HIP backend.
//
// Compiled with -fsyntax-only (tests/test_capi_materials.py) in two ways:
//   against the reference's headers: the application's own
//     std::vector<generic_material<plastic<float>, matte<float>, mirror<float>, emissive<float>>>
//     (generic_material.h, the model material of src/common/model.h:28) goes to hip_shading, which converts
//     every element through the reference's variant visitor and the materials' getters, and on to
//     make_hip_pathtracing_kernel; obj_loader.h fills a model of that material type;
//   with -DVRH_DROP_IN_STANDALONE and include/ alone: the same program over vrh_material records.
#ifndef VRH_DROP_IN_STANDALONE
#include <visionaray/math/math.h>
#include <visionaray/aligned_vector.h>
#include <visionaray/bvh.h>
#include <visionaray/camera.h>
#include <visionaray/generic_material.h>
#include <visionaray/material.h>
#include <visionaray/pixel_format.h>
#include <visionaray/point_light.h>
#include <visionaray/scheduler.h>
#include <visionaray/tags.h>

#include <visionaray_hip/hip_backend.h>
#else
#include <visionaray_hip/standalone.h>
#endif
#include <visionaray_hip/obj_loader.h>

#include <cstdio>
#include <vector>

using namespace visionaray;

#ifndef VRH_DROP_IN_STANDALONE
using material_t = generic_material<plastic<float>, matte<float>, mirror<float>, emissive<float>>;

// a model as src/common/model.h declares it, with the generic material type of model.h:28
struct generic_model
{
    using triangle_type = basic_triangle<3, float>;
    using normal_type = vector<3, float>;
    using tex_coord_type = vector<2, float>;
    using material_type = material_t;
    aligned_vector<triangle_type> primitives;
    aligned_vector<normal_type> shading_normals, geometric_normals;
    aligned_vector<tex_coord_type> tex_coords;
    aligned_vector<material_type> materials;
    aabb bbox;
};

static std::vector<material_t> make_materials()
{
    plastic<float> p;
    p.set_ca(from_rgb(vec3(0.0f, 0.0f, 0.0f))); p.set_ka(1.0f);
    p.set_cd(from_rgb(vec3(0.8f, 0.3f, 0.2f))); p.set_kd(1.0f);
    p.set_cs(from_rgb(vec3(1.0f, 1.0f, 1.0f))); p.set_ks(0.4f);
    p.set_specular_exp(32.0f);
    matte<float> m;
    m.set_ca(from_rgb(vec3(0.0f, 0.0f, 0.0f))); m.set_ka(1.0f);
    m.set_cd(from_rgb(vec3(0.8f, 0.8f, 0.8f))); m.set_kd(1.0f);
    mirror<float> r;
    r.set_cr(from_rgb(vec3(1.0f, 1.0f, 1.0f))); r.set_kr(0.9f);
    r.set_ior(spectrum<float>(from_rgb(vec3(0.2f, 0.9f, 1.1f))));
    r.set_absorption(spectrum<float>(from_rgb(vec3(3.9f, 2.4f, 2.2f))));
    emissive<float> e;
    e.set_ce(from_rgb(vec3(1.0f, 0.9f, 0.8f))); e.set_ls(8.0f);
    return { material_t(p), material_t(m), material_t(r), material_t(e) };
}
#else
using material_t = vrh_material;

static std::vector<material_t> make_materials()
{
    std::vector<material_t> m(2);
    m[0].kind = VRH_MATERIAL_MATTE;
    m[0].u.matte = { { 0.0f, 0.0f, 0.0f }, 1.0f, { 0.8f, 0.8f, 0.8f }, 1.0f };
    m[1].kind = VRH_MATERIAL_EMISSIVE;
    m[1].u.emissive = { { 1.0f, 0.9f, 0.8f }, 8.0f };
    return m;
}
#endif

int main(int argc, char** argv)
{
    using tri_t = basic_triangle<3, float>;
    std::vector<tri_t> tris(12);
    if (vrh_gen_cornell(tris.data()) != VRH_OK) return 2;
    std::vector<material_t> materials = make_materials();
    for (size_t i = 0; i < tris.size(); ++i) tris[i].geom_id = unsigned(i % materials.size());
    auto host_bvh = build<index_bvh<tri_t>>(tris.data(), tris.size());
    std::vector<vec4> normals(tris.size());
    if (vrh_face_normals(tris.data(), uint32_t(tris.size()), &normals[0].x) != VRH_OK) return 2;
    hip_index_bvh<tri_t> device_bvh(host_bvh, normals.data());

    std::vector<vrh_point_light> lights;
    hip_shading shading(materials, lights);

    hip_buffer_rt<PF_RGBA32F, PF_UNSPECIFIED> rt;
    rt.resize(64, 64);
    rt.clear_color_buffer();
    camera cam;
    cam.perspective(45.0f * constants::degrees_to_radians<float>(), 1.0f, 0.001f, 1000.0f);
    cam.look_at(vec3(0.0f, 0.0f, 3.0f), vec3(0.0f, 0.0f, 0.0f), vec3(0.0f, 1.0f, 0.0f));
    hip_sched<ray> sched;
    auto kernel = make_hip_pathtracing_kernel(normals_per_face_binding{}, device_bvh, shading,
                                              vec4(0.1f, 0.2f, 0.3f, 1.0f), vec4(0.0f, 0.0f, 0.0f, 0.0f), 5u, 1e-3f);
    auto sparams = make_sched_params(pixel_sampler::jittered_blend_type{}, cam, rt);
    sched.frame(kernel, sparams, 1);

#ifndef VRH_DROP_IN_STANDALONE
    if (argc > 1)
    {
        generic_model mod;
        load_obj(argv[1], mod);        // emissive<float> where the MTL file has a Ke, plastic<float> elsewhere
        hip_shading from_file(mod.materials, lights);
        printf("%zu materials, the first %s\n", mod.materials.size(), mod.materials[0].is_emissive() ? "emits" : "does not emit");
    }
#else
    if (argc > 1)
    {
        model mod;
        load_obj(argv[1], mod);
        printf("%zu materials\n", mod.materials.size());
    }
#endif
    return 0;
}
