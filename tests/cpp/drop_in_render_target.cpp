// tests/cpp/drop_in_render_target.cpp -- an application that keeps its render-target types on the HIP backend.
//
// Compiled with -fsyntax-only (tests/test_cpp_render_target.py) in two ways:
//   against the reference's headers: the reference's own pixel_format values (pixel_format.h) select the target --
//     the <PF_RGBA8, PF_UNSPECIFIED> of its volume / multi_volume / multi_hit / intersector / generic_primitive
//     examples, and a colour + depth target rendered through camera matrices;
//   with -DVRH_DROP_IN_STANDALONE and include/ alone: the same program over standalone.h's names.
#ifndef VRH_DROP_IN_STANDALONE
#include <visionaray/math/math.h>
#include <visionaray/bvh.h>
#include <visionaray/camera.h>
#include <visionaray/pixel_format.h>
#include <visionaray/scheduler.h>

#include <visionaray_hip/hip_backend.h>
#else
#include <visionaray_hip/standalone.h>
#endif

#include <cstdint>
#include <vector>

using namespace visionaray;

// the layouts the formats promise
static_assert(hip_buffer_rt<PF_RGBA8, PF_UNSPECIFIED>::formatted && hip_buffer_rt<PF_RGBA8, PF_UNSPECIFIED>::color_bytes == 4, "RGBA8");
static_assert(hip_buffer_rt<PF_RGB8, PF_DEPTH32F>::color_bytes == 3 && hip_buffer_rt<PF_RGB8, PF_DEPTH32F>::depth_format == VRH_DF_DEPTH32F, "RGB8");
static_assert(hip_buffer_rt<PF_RGB32F, PF_DEPTH24_STENCIL8>::color_bytes == 16, "RGB32F keeps the 16-byte vector<3, float>");
static_assert(hip_buffer_rt<PF_RGBA32F, PF_DEPTH32F>::formatted && !hip_buffer_rt<PF_RGBA32F, PF_UNSPECIFIED>::formatted, "the plain target");

int main()
{
    using tri_t = basic_triangle<3, float>;
    std::vector<tri_t> prims(1, tri_t(vec3(-1.0f, -1.0f, 0.0f), vec3(2.0f, 0.0f, 0.0f), vec3(0.0f, 2.0f, 0.0f)));
    prims[0].prim_id = 0; prims[0].geom_id = 0;
    auto host_bvh = build<index_bvh<tri_t>>(prims.data(), prims.size());
    std::vector<vec4> normals(1, vec4(0.0f, 0.0f, 1.0f, 0.0f));
    hip_index_bvh<tri_t> device_bvh(host_bvh, normals.data());
    const unsigned W = 64, H = 48;
    camera cam;
    cam.perspective(0.8f, W / static_cast<float>(H), 0.001f, 1000.0f);
    cam.look_at(vec3(0.0f, 0.0f, 3.0f), vec3(0.0f, 0.0f, 0.0f), vec3(0.0f, 1.0f, 0.0f));
    hip_sched<basic_ray<float>> sched;

    // cpu_buffer_rt<PF_RGBA8, PF_UNSPECIFIED> rt;  of the reference's examples
    hip_buffer_rt<PF_RGBA8, PF_UNSPECIFIED> rt;
    rt.resize(W, H);
    rt.clear_color_buffer(vec4(0.0f, 0.0f, 0.0f, 1.0f));
    sched.frame(make_hip_ao_kernel(device_bvh, vec4(0.1f, 0.2f, 0.3f, 1.0f)), make_sched_params(pixel_sampler::jittered_blend_type{}, cam, rt), 1);
    std::vector<uint8_t> rgba(size_t(W) * H * 4);
    rt.download_formatted(rgba.data());
    auto ref = rt.ref();
    (void)ref.formatted_color;

    // colour and depth through camera matrices, for compositing with rasterised geometry
    hip_buffer_rt<PF_RGB8, PF_DEPTH24_STENCIL8> rtd;
    rtd.resize(W, H);
    rtd.clear_depth_buffer();
    mat4 view = mat4::identity(), proj = mat4::identity();
    sched.frame(make_hip_closest_hit_kernel(device_bvh, vec4(0.0f, 0.0f, 0.0f, 1.0f)), make_sched_params(pixel_sampler::uniform_type{}, view, proj, rtd));
    std::vector<uint8_t> rgb(size_t(W) * H * 3);
    std::vector<uint32_t> depth(size_t(W) * H);
    rtd.download_formatted(rgb.data(), depth.data());
    return rtd.ref().depth != nullptr ? 0 : 1;
}
