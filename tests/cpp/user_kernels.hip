// tests/cpp/user_kernels.hip -- user kernels and custom intersectors through hip_sched::frame
// (include/visionaray_hip/hip_kernels.h), compiled by hipcc (visionaray_amd/Makefile `cpp_tests`).
//
//   user_kernels ao    <grid> <W> <H> <outdir> [frame]          AO kernel written as a device lambda,
//                                                               default intersector
//   user_kernels mask  <grid> <W> <H> <outdir> <mask.bin> <n>   the same kernel with a byte-mask
//                                                               basic_intersector (the reference
//                                                               harness's "mask" intersector)
//   user_kernels heart <grid> <W> <H> <outdir>                  closest hit with the intersector
//                                                               example's procedural heart cut-out
//   user_kernels isect <grid> <W> <H> <outdir> <mask.bin> <n>   the mask case with the intersector in the
//                                                                sched params: kernel(isect, r, x, y)
//   user_kernels sampler <grid> <W> <H> <outdir> <kind> <frame> the harness's sampler frames (jittered,
//                                                                jittered_blend, ssaa2/4/8) with a user kernel
//   user_kernels list  <grid> <W> <H> <outdir> x0 y0 x1 y1 f    the AO kernel over a list of two BVHs
//                                                               (prim_id parity split), scissor box,
//                                                               frame f (the harness's "list" mode)
//   user_kernels bench <grid> <W> <H> <outdir> [launches] [F]   throughput of the AO user kernel (F > 1:
//                                                                F frames per hip_sched::frames launch)
//   user_kernels frames <grid> <W> <H> <outdir> [frame]         frames in flight: three cameras in one
//                                                                frames() launch equal three frame() calls
//   user_kernels draws <grid> <W> <H> <outdir> <frame>          kernel(r, random_sampler<float>&): draws
//                                                                0, 1, 2, 15 of the pixel's sampler as colour
//   user_kernels anyrec <grid> <W> <H> <outdir> <frame> [radius] the AO lambda's any_hit hit records, hashed
//   user_kernels chain <grid> <W> <H> <outdir> <frame> [radius] any_hit calls that depend on earlier answers
//   user_kernels rsao  <grid> <W> <H> <outdir> <frame>          the AO example's kernel (ao/main.cpp:183-246)
//                                                                with standalone.h's random_sampler and
//                                                                cosine_sample_hemisphere; depth = hit t
//   user_kernels deep  <grid> <W> <H> <outdir> <scenedir> <route>  the AO kernel on a BVH read from files
//                                                                (nodes.bin, prims.bin, indices.bin,
//                                                                normals.bin, cam.bin: eye, center, up;
//                                                                tests/deep_cases.py), the hip_bvh_ref made
//                                                                by <route>:
//                                                                  ref      checked_ref(device_bvh.ref())
//                                                                  checked  vrh_scene_get_view + checked_ref
//                                                                  view     vrh_scene_get_view alone
//                                                                  grow     hf<grid> through ref() (24 stack
//                                                                           entries), then the BVH's ref()
//                                                                           (depth + 1 entries) and its frame
//                                                                  recover  route view, the error expected;
//                                                                           then checked_ref on the same view
//                                                                           and the frame
//                                                                a hip_error: {"error_status": ..} and exit
//                                                                status 3 (1: any other failure)
//
// The kernel is the reference harness's AO lambda (oracle/ref_harness.cpp run_golden, after
// ao/main.cpp:183-246) as a user would port it to cuda_sched: closest_hit over the BVH refs, the
// face normal, make_orthonormal_basis, 8 samples, any_hit with radius 0.1.  Its colour channels
// carry the outputs the tests compare bit for bit with the reference's frames: x = prim id bits,
// y = t, z = occlusion mask bits, w = the AO grey value (bg.w on a miss).  Writes prim_id.bin,
// t.bin, occ.bin, color.bin (RGBA32F as the reference stores it) into outdir.
#include <visionaray_hip/hip_kernels.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace visionaray;

//-------------------------------------------------------------------------------------------------
// a byte mask over the hit's texture coordinate (nearest texel), as the harness's mask_intersector
//

struct byte_mask_intersector : basic_intersector<byte_mask_intersector>
{
    using basic_intersector<byte_mask_intersector>::operator();

    template <typename R, typename S>
    __device__ auto operator()(R const& ray, basic_triangle<3, S> const& tri) -> decltype(intersect(ray, tri))
    {
        auto hr = intersect(ray, tri);
        if (!hr.hit) return hr;
        vec2 tc = get_tex_coord(tex_coords, hr);
        hr.hit &= mask[texel(tc.y, h) * unsigned(w) + texel(tc.x, w)] != 0;
        return hr;
    }

    __device__ static unsigned texel(float c, int n)
    {
        float x = (c > 0.0f ? c : 0.0f) * float(n);
        return x < float(n) ? unsigned(x) : unsigned(n - 1);
    }

    vec2 const* tex_coords = nullptr;
    uint8_t const* mask = nullptr;
    int w = 0, h = 0;
};

//-------------------------------------------------------------------------------------------------
// The intersector example's procedural cut-out, written in its width-generic style (the same code
// serves float, float4 and float8 rays on the CPU): host code without VSNRAY_FUNC becomes device
// code inside the force_cuda_host_device region.
//

#pragma clang force_cuda_host_device begin
struct heart_intersector : basic_intersector<heart_intersector>
{
    using basic_intersector<heart_intersector>::operator();

    template <typename R, typename S>
    auto operator()(R const& ray, basic_triangle<3, S> const& tri) -> decltype(intersect(ray, tri))
    {
        using T = typename R::scalar_type;
        static const int N = simd::num_elements<T>::value;
        using Mask = simd::mask_type_t<T>;

        assert(tex_coords);
        auto hr = intersect(ray, tri);
        if (!any(hr.hit))
        {
            return hr;
        }
        auto tc = get_tex_coord(tex_coords, hr);
        auto hrs = unpack(hr);
        auto tcs = unpack(tc);

        bool keep[N];
        memset(keep, 0, sizeof(keep));
        for (int i = 0; i < N; ++i)
        {
            if (!hrs[i].hit) continue;
            auto x = tcs[i].x * 3.0f - 1.5f;
            auto y = tcs[i].y * 3.0f - 1.5f;
            keep[i] = (pow(x * x + y * y - 1.0f, 3.0f) - x * x * y * y * y) < 0.0f;
        }
        hr.hit &= Mask(keep);
        return hr;
    }

    vec2 const* tex_coords;
};
#pragma clang force_cuda_host_device end

static void write_file(std::string const& path, const void* p, size_t n)
{
    FILE* f = fopen(path.c_str(), "wb");
    if (!f || fwrite(p, 1, n, f) != n) { fprintf(stderr, "cannot write %s\n", path.c_str()); exit(3); }
    fclose(f);
}

template <typename T>
static T* to_device(std::vector<T> const& v)
{
    T* d = nullptr;
    if (hipMalloc(&d, v.size() * sizeof(T)) != hipSuccess ||
        hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess)
    {
        fprintf(stderr, "device copy failed\n");
        exit(4);
    }
    return d;
}

// a short list of BVH refs (the bvh_ref vector of ao/main.cpp:171-178) in device memory, as the
// reference's GPU programs hold them (a thrust::device_vector<bvh_ref> whose begin / end the kernel
// captures; a by-value array in the lambda would be copied to scratch memory per thread)
struct ref_list
{
    hip_bvh_ref const* r;
    unsigned n;
};

// primary closest hit + 8 AO samples with intersector `isect` over the BVH list `refs`
// (oracle/ref_harness.cpp run_golden / run_list)
template <typename Isect>
__device__ static result_record<float> ao_body(ref_list refs, vec3 const* normals, Isect& isect, unsigned W,
                                              unsigned frame_num, ray r, unsigned x, unsigned y)
{
    result_record<float> result;
    const vec4 bg(0.1f, 0.2f, 0.3f, 1.0f);
    result.color = vec4(__uint_as_float(0xFFFFFFFFu), -1.0f, 0.0f, bg.w);
    hip_bvh_ref const* begin = refs.r;
    hip_bvh_ref const* end = refs.r + refs.n;
    auto hr = closest_hit(r, begin, end, isect);
    result.hit = hr.hit;
    if (!hr.hit) return result;
    hr.isect_pos = r.ori + r.dir * hr.t;
    float clr = 1.0f;
    vec3 n = get_normal(normals, hr);
    vec3 uu, vv, w = n;
    make_orthonormal_basis(uu, vv, w);
    unsigned mask = 0;
    const unsigned p = y * W + x;
    for (unsigned smp = 0; smp < 8; ++smp)
    {
        vec3 s = hip_ao_sample(p, smp, frame_num);
        auto dir = normalize(s.x * uu + s.y * vv + s.z * w);
        ray ao(hr.isect_pos + dir * 1E-3f, dir);
        auto ar = any_hit(ao, begin, end, 0.1f, isect);
        if (ar.hit) { clr = clr - 1.0f / 8; mask |= 1u << smp; }
    }
    result.color = vec4(__uint_as_float(unsigned(hr.prim_id)), hr.t, __uint_as_float(mask), clr);
    return result;
}

template <typename Isect>
static auto ao_kernel(ref_list refs, vec3 const* normals, Isect isect, unsigned W, unsigned frame_num)
{
    return [=] __device__ (ray r, unsigned x, unsigned y) mutable -> result_record<float>
    {
        return ao_body(refs, normals, isect, W, frame_num, r, x, y);
    };
}

// primary closest hit only: prim id and t
template <typename Isect>
static auto primary_kernel(hip_bvh_ref ref, Isect isect)
{
    return [=] __device__ (ray r) mutable -> result_record<float>
    {
        result_record<float> result;
        result.color = vec4(__uint_as_float(0xFFFFFFFFu), -1.0f, 0.0f, 1.0f);
        auto hr = closest_hit(r, &ref, &ref + 1, isect);
        if (hr.hit) result.color = vec4(__uint_as_float(unsigned(hr.prim_id)), hr.t, 0.0f, 1.0f);
        result.hit = hr.hit;
        return result;
    };
}

// the reference harness's `sampler` kernel (oracle/ref_harness.cpp run_sampler_impl): bg on a miss,
// (1 - k/8, 1 - k/8, 1 - k/8, 1) for k occluded AO samples on a hit; the last sample's prim id
static auto sampler_kernel(ref_list refs, vec3 const* normals, uint32_t* pid, unsigned W, unsigned frame_num)
{
    return [=] __device__ (ray r, unsigned x, unsigned y) -> result_record<float>
    {
        result_record<float> result;
        result.color = vec4(0.1f, 0.2f, 0.3f, 1.0f);
        default_intersector isect;
        hip_bvh_ref const* begin = refs.r;
        hip_bvh_ref const* end = refs.r + refs.n;
        auto hr = closest_hit(r, begin, end, isect);
        result.hit = hr.hit;
        const unsigned p = y * W + x;
        pid[p] = hr.hit ? unsigned(hr.prim_id) : 0xFFFFFFFFu;
        if (!hr.hit) return result;
        hr.isect_pos = r.ori + r.dir * hr.t;
        float clr = 1.0f;
        vec3 n = get_normal(normals, hr);
        vec3 uu, vv, w = n;
        make_orthonormal_basis(uu, vv, w);
        for (unsigned smp = 0; smp < 8; ++smp)
        {
            vec3 s = hip_ao_sample(p, smp, frame_num);
            auto dir = normalize(s.x * uu + s.y * vv + s.z * w);
            ray ao(hr.isect_pos + dir * 1E-3f, dir);
            if (any_hit(ao, begin, end, 0.1f, isect).hit) clr = clr - 1.0f / 8;
        }
        result.color = vec4(clr, clr, clr, 1.0f);
        return result;
    };
}

// the AO kernel with the intersector taken from the sched params: kernel(isect, r, x, y)
static auto ao_kernel_isect(ref_list refs, vec3 const* normals, unsigned W, unsigned frame_num)
{
    return [=] __device__ (byte_mask_intersector& isect, ray r, unsigned x, unsigned y) -> result_record<float>
    {
        return ao_body(refs, normals, isect, W, frame_num, r, x, y);
    };
}

// the AO lambda's frame `out` (RGBA32F as rendered) decoded into the reference's four outputs:
// prim_id.bin, t.bin, occ.bin, color.bin; box: the scissor box (x0, y0, x1, y1)
static void write_outputs(std::string const& outdir, std::string const& mode, unsigned W, unsigned H,
                          std::vector<float> const& out, const int (&box)[4])
{
    const size_t npx = size_t(W) * H;
    std::vector<uint32_t> pid(npx);
    std::vector<float> t(npx), color(4 * npx);
    std::vector<uint8_t> occ(npx);
    for (size_t p = 0; p < npx; ++p)
    {
        uint32_t bits;
        memcpy(&bits, &out[4 * p], 4);
        pid[p] = bits;
        t[p] = out[4 * p + 1];
        memcpy(&bits, &out[4 * p + 2], 4);
        occ[p] = uint8_t(bits);
        const float g = out[4 * p + 3];
        const bool hit = pid[p] != 0xFFFFFFFFu;
        const float c[4] = { hit ? g : 0.1f, hit ? g : 0.2f, hit ? g : 0.3f, 1.0f };
        memcpy(&color[4 * p], c, 16);
        const int px = int(p % W), py = int(p / W);
        if (px < box[0] || py < box[1] || px >= box[2] || py >= box[3])
        {
            // outside the scissor box: the cleared target, as the reference leaves it
            pid[p] = 0xFFFFFFFFu; t[p] = -1.0f; occ[p] = 0;
            memset(&color[4 * p], 0, 16);
        }
    }
    write_file(outdir + "/prim_id.bin", pid.data(), npx * 4);
    write_file(outdir + "/t.bin", t.data(), npx * 4);
    write_file(outdir + "/occ.bin", occ.data(), npx);
    write_file(outdir + "/color.bin", color.data(), npx * 16);
    size_t hits = 0;
    for (auto p : pid) hits += p != 0xFFFFFFFFu;
    printf("{\"mode\":\"%s\",\"W\":%u,\"H\":%u,\"hits\":%zu}\n", mode.c_str(), W, H, hits);
}

// a hip_error (a status of the library, or of the headers: VRH_ERR_UNSUPPORTED for a BVH deeper than the
// traversal stack): one JSON line with the status, exit status 3; any other failure exits with 1
static int report_hip_error(hip_error const& e)
{
    std::string what;
    for (const char* c = e.what(); *c; ++c)
    {
        if (*c == '"' || *c == '\\') { what += '\\'; what += *c; }
        else what += (unsigned char)(*c) < 0x20 ? ' ' : *c;
    }
    printf("{\"error_status\":%d,\"what\":\"%s\",\"stack_entries\":%u}\n", e.status, what.c_str(),
           visionaray::hip_detail::last_user_launch().stack_entries);
    fflush(stdout);
    fprintf(stderr, "error: %s\n", e.what());
    return 3;
}

template <typename T>
static std::vector<T> read_file(std::string const& path)
{
    std::vector<T> v;
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", path.c_str()); exit(2); }
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (n < 0 || size_t(n) % sizeof(T) != 0) { fprintf(stderr, "%s: not a whole number of records\n", path.c_str()); exit(2); }
    v.resize(size_t(n) / sizeof(T));
    if (fread(static_cast<void*>(v.data()), sizeof(T), v.size(), f) != v.size()) { fprintf(stderr, "cannot read %s\n", path.c_str()); exit(2); }
    fclose(f);
    return v;
}

// deep <grid> W H outdir <scenedir> <route>: the AO lambda over a BVH handed in as files, so that the
// test decides the tree (deeper than the short LDS stack, or than the whole one) and the oracle renders
// the same bytes.  The route is how the hip_bvh_ref the lambda captures is made (the head of this file).
static int run_deep(int argc, char** argv, unsigned grid, unsigned W, unsigned H, std::string const& outdir)
{
    if (argc < 8) return 2;
    const std::string dir = argv[6], route = argv[7];
    using tri_t = basic_triangle<3, float>;
    const auto prims = read_file<tri_t>(dir + "/prims.bin");
    index_bvh<tri_t> host(prims.data(), prims.size());
    host.nodes() = read_file<bvh_node>(dir + "/nodes.bin");
    host.indices() = read_file<unsigned>(dir + "/indices.bin");
    const auto normals = read_file<vec4>(dir + "/normals.bin");
    const auto cf = read_file<float>(dir + "/cam.bin");
    if (normals.size() != prims.size() || cf.size() != 9) { fprintf(stderr, "deep: normals.bin / cam.bin size\n"); return 2; }
    try
    {
        hip_index_bvh<tri_t> dev(host, normals.data());         // vrh_scene_upload computes the depth
        hip_buffer_rt<PF_RGBA32F, PF_UNSPECIFIED> rt;
        rt.resize(W, H);
        camera cam;
        cam.perspective(45.0f * constants::degrees_to_radians<float>(), W / static_cast<float>(H), 0.001f, 1000.0f);
        cam.look_at(vec3(cf[0], cf[1], cf[2]), vec3(cf[3], cf[4], cf[5]), vec3(cf[6], cf[7], cf[8]));
        hip_sched<ray> sched;
        std::vector<float> out(4 * size_t(W) * H);
        auto const& li = visionaray::hip_detail::last_user_launch();
        // one frame of the AO lambda over r with camera c; the download waits for it
        auto render = [&](hip_bvh_ref const& r, camera const& c)
        {
            auto sp = make_sched_params(pixel_sampler::uniform_type{}, c, rt);
            const ref_list one{ to_device(std::vector<hip_bvh_ref>{ r }), 1u };
            sched.frame(ao_kernel(one, static_cast<vec3 const*>(r.view.normals), default_intersector{}, W, 0u), sp);
            rt.download(out.data());
        };
        auto plain_view = [&]()
        {
            hip_bvh_ref r{};
            hip_detail::check(vrh_scene_get_view(dev.handle(), 0, &r.view), "vrh_scene_get_view");
            return r;
        };
        unsigned first_entries = 0;
        int first_status = 0;
        uint32_t depth = 0;
        if (route == "ref")
        {
            hip_bvh_ref r = checked_ref(dev.ref());
            depth = r.view.max_depth;
            render(r, cam);
        }
        else if (route == "checked")
        {
            hip_bvh_ref r = plain_view();
            depth = r.view.max_depth;
            render(checked_ref(r), cam);
        }
        else if (route == "view")
        {
            hip_bvh_ref r = plain_view();
            depth = r.view.max_depth;
            render(r, cam);
        }
        else if (route == "grow")
        {
            // a shallow BVH first: the launch takes the short stack; then the first ref() of the deep one
            std::vector<tri_t> tris(size_t(2) * grid * grid);
            if (vrh_gen_heightfield(grid, tris.data()) != VRH_OK) return 2;
            auto hf = build<index_bvh<tri_t>>(tris.data(), tris.size());
            std::vector<vec4> hn(tris.size());
            if (vrh_face_normals(tris.data(), uint32_t(tris.size()), &hn[0].x) != VRH_OK) return 2;
            hip_index_bvh<tri_t> hf_dev(hf, hn.data());
            camera hcam = cam;
            hcam.look_at(vec3(0.0f, 0.9f, 1.4f), vec3(0.0f, 0.0f, 0.0f), vec3(0.0f, 1.0f, 0.0f));
            render(checked_ref(hf_dev.ref()), hcam);
            first_entries = li.stack_entries;
            hip_bvh_ref r = checked_ref(dev.ref());
            depth = r.view.max_depth;
            render(r, cam);
        }
        else if (route == "recover")
        {
            // the unregistered view: the walk is declined and the download reports it, once; the same view
            // through checked_ref then renders on the same context and target
            hip_bvh_ref r = plain_view();
            depth = r.view.max_depth;
            try
            {
                render(r, cam);
                fprintf(stderr, "recover: the unregistered view of a BVH %u deep rendered without an error\n", depth);
                return 1;
            }
            catch (hip_error const& e)
            {
                first_status = e.status;
                first_entries = li.stack_entries;
            }
            hip_context::default_context()->sync();             // reported once: nothing left to throw
            render(checked_ref(r), cam);
        }
        else
            return 2;
        printf("{\"mode\":\"deep\",\"route\":\"%s\",\"max_depth\":%u,\"stack_entries\":%u,\"first_stack_entries\":%u,"
               "\"first_error_status\":%d}\n", route.c_str(), depth, li.stack_entries, first_entries, first_status);
        const int box[4] = { 0, 0, int(W), int(H) };
        write_outputs(outdir, "deep", W, H, out, box);
    }
    catch (hip_error const& e)
    {
        return report_hip_error(e);
    }
    catch (std::exception const& e)
    {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 6) { fprintf(stderr, "usage: user_kernels ao|mask|heart grid W H outdir ...\n"); return 2; }
    const std::string mode = argv[1];
    const unsigned grid = unsigned(atoi(argv[2])), W = unsigned(atoi(argv[3])), H = unsigned(atoi(argv[4]));
    const std::string outdir = argv[5];
    if (mode == "deep") return run_deep(argc, argv, grid, W, H, outdir);
    using tri_t = basic_triangle<3, float>;
    std::vector<tri_t> tris(size_t(2) * grid * grid);
    if (vrh_gen_heightfield(grid, tris.data()) != VRH_OK) return 2;
    auto host_bvh = build<index_bvh<tri_t>>(tris.data(), tris.size());
    std::vector<vec4> normals(tris.size());
    if (vrh_face_normals(tris.data(), uint32_t(tris.size()), &normals[0].x) != VRH_OK) return 2;
    // planar (x, z) texture coordinates of every corner, per prim_id (as the harness's mask mode)
    std::vector<vec2> tc(3 * tris.size());
    for (auto const& t : tris)
    {
        vec3 c[3] = { t.v1, t.v1 + t.e1, t.v1 + t.e2 };
        for (int k = 0; k < 3; ++k) tc[3 * t.prim_id + k] = vec2(c[k].x * 0.5f + 0.5f, c[k].z * 0.5f + 0.5f);
    }

    try
    {
        hip_index_bvh<tri_t> device_bvh(host_bvh, normals.data());
        hip_buffer_rt<PF_RGBA32F, PF_UNSPECIFIED> rt;
        rt.resize(W, H);
        camera cam;
        cam.perspective(45.0f * constants::degrees_to_radians<float>(), W / static_cast<float>(H), 0.001f, 1000.0f);
        cam.look_at(vec3(0.0f, 0.9f, 1.4f), vec3(0.0f, 0.0f, 0.0f), vec3(0.0f, 1.0f, 0.0f));
        hip_sched<ray> sched;
        auto sparams = make_sched_params(pixel_sampler::uniform_type{}, cam, rt);
        hip_bvh_ref ref = checked_ref(device_bvh.ref());
        vec3 const* dnormals = static_cast<vec3 const*>(ref.view.normals);
        vec2* dtc = to_device(tc);
        const ref_list one{ to_device(std::vector<hip_bvh_ref>{ ref }), 1u };
        int box[4] = { 0, 0, int(W), int(H) };      // list mode: the scissor box (x0, y0, x1, y1)

        if (mode == "ao")
        {
            unsigned frame_num = argc > 6 ? unsigned(strtoul(argv[6], nullptr, 10)) : 0u;
            sched.frame(ao_kernel(one, dnormals, default_intersector{}, W, frame_num), sparams, frame_num);
        }
        else if (mode == "draws")
        {
            const unsigned frame_num = unsigned(strtoul(argv[6], nullptr, 10));
            sched.frame([=] __device__ (ray r, random_sampler<float>& samp) -> result_record<float>
            {
                result_record<float> result;
                float d[16];
                for (int k = 0; k < 16; ++k) d[k] = samp.next();
                result.color = vec4(d[0], d[1], d[2], d[15]);
                return result;
            }, sparams, frame_num);
            std::vector<float> out(4 * size_t(W) * H);
            rt.download(out.data());
            write_file(outdir + "/color.bin", out.data(), out.size() * 4);
            return 0;
        }
        else if (mode == "rsao")
        {
            const unsigned frame_num = unsigned(strtoul(argv[6], nullptr, 10));
            hip_bvh_ref const* begin = one.r;
            hip_bvh_ref const* end = one.r + one.n;
            sched.frame([=] __device__ (ray r, random_sampler<float>& samp) -> result_record<float>
            {
                result_record<float> result;
                result.color = vec4(0.1f, 0.2f, 0.3f, 1.0f);
                auto hr = closest_hit(r, begin, end);
                result.hit = hr.hit;
                if (hr.hit)
                {
                    hr.isect_pos = r.ori + r.dir * hr.t;
                    result.depth = hr.t;
                    vec4 clr(1.0f);
                    vec3 n = get_normal(dnormals, hr);
                    vec3 u, v, w = n;
                    make_orthonormal_basis(u, v, w);
                    for (int i = 0; i < 8; ++i)
                    {
                        auto sp = cosine_sample_hemisphere(samp.next(), samp.next());
                        auto dir = normalize(sp.x * u + sp.y * v + sp.z * w);
                        ray ao(hr.isect_pos + dir * 1E-3f, dir);
                        if (any_hit(ao, begin, end, 0.1f).hit) clr = clr - 1.0f / 8;
                    }
                    result.color = vec4(clr.x, clr.y, clr.z, 1.0f);
                }
                return result;
            }, sparams, frame_num);
            std::vector<float> out(4 * size_t(W) * H), t(size_t(W) * H);
            rt.download(out.data(), nullptr, t.data());
            write_file(outdir + "/color.bin", out.data(), out.size() * 4);
            write_file(outdir + "/t.bin", t.data(), t.size() * 4);
            return 0;
        }
        else if (mode == "anyrec")
        {
            // the hit RECORDS of the AO lambda's any_hit calls, not only hit / miss: per pixel an
            // FNV-1a hash over (hit, prim_id, t bits) of the 8 records (colour x), the number of hits
            // (colour y) -- any_hit returns the first hit in the walk's visiting order, so a build
            // with the entry cut (VRH_USER_ANYHIT_CUT) must give the records of the build without it
            const unsigned frame_num = unsigned(strtoul(argv[6], nullptr, 10));
            const float radius = argc > 7 ? float(atof(argv[7])) : 0.1f;
            hip_bvh_ref const* begin = one.r;
            hip_bvh_ref const* end = one.r + one.n;
            sched.frame([=] __device__ (ray r, random_sampler<float>& samp) -> result_record<float>
            {
                result_record<float> result;
                result.color = vec4(0.0f, 0.0f, 0.0f, 0.0f);
                auto hr = closest_hit(r, begin, end);
                if (hr.hit)
                {
                    hr.isect_pos = r.ori + r.dir * hr.t;
                    vec3 n = get_normal(dnormals, hr);
                    vec3 u, v, w = n;
                    make_orthonormal_basis(u, v, w);
                    uint32_t h = 2166136261u, hits = 0;
                    auto mix = [&](uint32_t x) { for (int k = 0; k < 4; ++k) { h ^= (x >> (8 * k)) & 0xFFu; h *= 16777619u; } };
                    for (int i = 0; i < 8; ++i)
                    {
                        auto sp = cosine_sample_hemisphere(samp.next(), samp.next());
                        auto dir = normalize(sp.x * u + sp.y * v + sp.z * w);
                        ray ao(hr.isect_pos + dir * 1E-3f, dir);
                        auto rec = any_hit(ao, begin, end, radius);
                        mix(rec.hit ? 1u : 0u);
                        if (rec.hit) { mix(uint32_t(rec.prim_id)); mix(__float_as_uint(rec.t)); hits += 1u; }
                    }
                    result.color = vec4(__uint_as_float(h), float(hits), 1.0f, 1.0f);
                }
                return result;
            }, sparams, frame_num);
            std::vector<float> out(4 * size_t(W) * H);
            rt.download(out.data());
            write_file(outdir + "/color.bin", out.data(), out.size() * 4);
            return 0;
        }
        else if (mode == "chain")
        {
            // chain <grid> W H outdir frame radius: a kernel whose calls depend on earlier answers -- per
            // AO sample an any_hit; when it hits, two more any_hit calls (a shorter and a reflected ray).
            // Under VRH_USER_DEFER the record phase sees every first call answered "no hit" (pending) and
            // logs one call per sample; the replay, with the real answers, makes up to three: the calls
            // past the record phase's count must run directly, not read the log slots an earlier tile
            // left.  The frame (a hash of every record, the number of calls) must equal the
            // direct build's.
            const unsigned frame_num = unsigned(strtoul(argv[6], nullptr, 10));
            const float radius = argc > 7 ? float(atof(argv[7])) : 0.1f;
            hip_bvh_ref const* begin = one.r;
            hip_bvh_ref const* end = one.r + one.n;
            sched.frame([=] __device__ (ray r, random_sampler<float>& samp) -> result_record<float>
            {
                result_record<float> result;
                result.color = vec4(0.0f, 0.0f, 0.0f, 0.0f);
                auto hr = closest_hit(r, begin, end);
                if (hr.hit)
                {
                    hr.isect_pos = r.ori + r.dir * hr.t;
                    vec3 n = get_normal(dnormals, hr);
                    vec3 u, v, w = n;
                    make_orthonormal_basis(u, v, w);
                    uint32_t h = 2166136261u, calls = 0;
                    auto mix = [&](uint32_t x) { for (int k = 0; k < 4; ++k) { h ^= (x >> (8 * k)) & 0xFFu; h *= 16777619u; } };
                    auto rec_mix = [&](decltype(hr) const& rec) {
                        mix(rec.hit ? 1u : 0u);
                        if (rec.hit) { mix(uint32_t(rec.prim_id)); mix(__float_as_uint(rec.t)); }
                    };
                    for (int i = 0; i < 4; ++i)
                    {
                        auto sp = cosine_sample_hemisphere(samp.next(), samp.next());
                        auto dir = normalize(sp.x * u + sp.y * v + sp.z * w);
                        ray ao(hr.isect_pos + dir * 1E-3f, dir);
                        auto rec = any_hit(ao, begin, end, radius);
                        rec_mix(rec);
                        calls += 1u;
                        if (rec.hit)
                        {
                            rec_mix(any_hit(ao, begin, end, rec.t * 0.5f));
                            auto refl = normalize(dir - n * (2.0f * dot(dir, n)));
                            rec_mix(any_hit(ray(hr.isect_pos + n * 1E-3f, normalize(refl + n)), begin, end, radius));
                            calls += 2u;
                        }
                    }
                    result.color = vec4(__uint_as_float(h), float(calls), 1.0f, 1.0f);
                }
                return result;
            }, sparams, frame_num);
            std::vector<float> out(4 * size_t(W) * H);
            rt.download(out.data());
            write_file(outdir + "/color.bin", out.data(), out.size() * 4);
            return 0;
        }
        else if (mode == "sphrec")
        {
            // sphrec <grid> W H outdir frame radius n: a sphere scene (vrh_gen_spheres: n spheres in
            // [-1, 1]^3, the camera at (0, 0, 3.5) as scenes.py's sph<n>): per pixel the closest hit
            // (prim id, t) and an FNV-1a hash over the records of 8 any_hit rays of radius `radius`
            // from the hit point (a hemisphere about -dir) -- the sphere path of closest_hit / any_hit,
            // and of the deferred build's trace
            const unsigned frame_num = unsigned(strtoul(argv[6], nullptr, 10));
            const float radius = float(atof(argv[7]));
            const unsigned nsph = unsigned(strtoul(argv[8], nullptr, 10));
            using sph_t = basic_sphere<float>;
            std::vector<sph_t> sph(nsph);
            if (vrh_gen_spheres(nsph, sph.data()) != VRH_OK) return 2;
            auto host_sph = build<index_bvh<sph_t>>(sph.data(), sph.size());
            hip_index_bvh<sph_t> dev_sph(host_sph);
            hip_bvh_ref sref = checked_ref(dev_sph.ref());

            const ref_list sl{ to_device(std::vector<hip_bvh_ref>{ sref }), 1u };
            camera scam;
            scam.perspective(45.0f * constants::degrees_to_radians<float>(), W / static_cast<float>(H), 0.001f, 1000.0f);
            scam.look_at(vec3(0.0f, 0.0f, 3.5f), vec3(0.0f, 0.0f, 0.0f), vec3(0.0f, 1.0f, 0.0f));
            auto sp_params = make_sched_params(pixel_sampler::uniform_type{}, scam, rt);
            hip_bvh_ref const* begin = sl.r;
            hip_bvh_ref const* end = sl.r + sl.n;
            sched.frame([=] __device__ (ray r, random_sampler<float>& samp) -> result_record<float>
            {
                result_record<float> result;
                result.color = vec4(0.0f, 0.0f, __uint_as_float(0xFFFFFFFFu), -1.0f);
                auto hr = closest_hit(r, begin, end);
                if (hr.hit)
                {
                    const vec3 p = r.ori + r.dir * hr.t;
                    vec3 u, v, w = normalize(-r.dir);
                    make_orthonormal_basis(u, v, w);
                    uint32_t h = 2166136261u, hits = 0;
                    auto mix = [&](uint32_t x) { for (int k = 0; k < 4; ++k) { h ^= (x >> (8 * k)) & 0xFFu; h *= 16777619u; } };
                    for (int i = 0; i < 8; ++i)
                    {
                        auto sp = cosine_sample_hemisphere(samp.next(), samp.next());
                        auto dir = normalize(sp.x * u + sp.y * v + sp.z * w);
                        auto rec = any_hit(ray(p + dir * 1E-3f, dir), begin, end, radius);
                        mix(rec.hit ? 1u : 0u);
                        if (rec.hit) { mix(uint32_t(rec.prim_id)); mix(__float_as_uint(rec.t)); hits += 1u; }
                    }
                    result.color = vec4(__uint_as_float(h), float(hits), __uint_as_float(uint32_t(hr.prim_id)), hr.t);
                }
                return result;
            }, sp_params, frame_num);
            std::vector<float> out(4 * size_t(W) * H);
            rt.download(out.data());
            write_file(outdir + "/color.bin", out.data(), out.size() * 4);
            return 0;
        }
        else if (mode == "bench")
        {
            // user-kernel throughput, median wall time per frame over `launches` synchronous launches:
            //   F = 1: the AO lambda (hip_ao_sample, the built-in sample set), one frame() per frame as
            //          cuda_sched is driven;
            //   F > 1: the AO lambda drawing its directions from the per-pixel random_sampler (distinct
            //          samples per frame number), F frames per frames() launch
            const int launches = argc > 6 ? atoi(argv[6]) : 10;
            const int F = argc > 7 ? atoi(argv[7]) : 1;
            hip_bvh_ref const* begin = one.r;
            hip_bvh_ref const* end = one.r + one.n;
            auto rs_ao = [=] __device__ (ray r, random_sampler<float>& samp) -> result_record<float>
            {
                result_record<float> result;
                result.color = vec4(0.1f, 0.2f, 0.3f, 1.0f);
                auto hr = closest_hit(r, begin, end);
                result.hit = hr.hit;
                if (hr.hit)
                {
                    hr.isect_pos = r.ori + r.dir * hr.t;
                    float clr = 1.0f;
                    vec3 n = get_normal(dnormals, hr);
                    vec3 u, v, w = n;
                    make_orthonormal_basis(u, v, w);
                    for (int i = 0; i < 8; ++i)
                    {
                        auto sp = cosine_sample_hemisphere(samp.next(), samp.next());
                        auto dir = normalize(sp.x * u + sp.y * v + sp.z * w);
                        ray ao(hr.isect_pos + dir * 1E-3f, dir);
                        if (any_hit(ao, begin, end, 0.1f).hit) clr = clr - 1.0f / 8;
                    }
                    result.color = vec4(clr, clr, clr, 1.0f);
                }
                return result;
            };
            hip_buffer_rt<PF_RGBA32F, PF_UNSPECIFIED> rtF;
            rtF.resize(W, H * unsigned(F));
            std::vector<camera> cams(size_t(F), cam);
            std::vector<double> ms;
            for (int l = 0; l <= launches; ++l)
            {
                auto t0 = std::chrono::steady_clock::now();
                if (F == 1) sched.frame(ao_kernel(one, dnormals, default_intersector{}, W, unsigned(l)), sparams, unsigned(l));
                else sched.frames(rs_ao, cams, rtF, unsigned(l * F));
                hip_context::default_context()->sync();     // frame() only issues the launch (cuda_sched's model)
                auto t1 = std::chrono::steady_clock::now();
                if (l > 0) ms.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count() / F);
            }
            std::sort(ms.begin(), ms.end());
            const auto& li = visionaray::hip_detail::last_user_launch();
            printf("{\"mode\":\"bench\",\"frame_ms_median\":%.4f,\"launches\":%d,\"frames_per_launch\":%d,"
                   "\"kernel\":\"%s\",\"launch\":{\"waves_target\":%d,\"blocks_per_cu\":%d,\"stack_entries\":%u,\"grid\":%u}}\n",
                   ms[ms.size() / 2], launches, F, F == 1 ? "ao lambda" : "random_sampler ao lambda",
                   li.waves_target, li.blocks_per_cu, li.stack_entries, li.grid);
#if VRH_DEFER_PROF
            {
                // the blocks' phase counters at the head of their logs (hip_kernels.h VRH_DEFER_PROF)
                auto& sb = hip_context::default_context()->scratch();
                std::vector<unsigned long long> h(sb.bytes / 8);
                (void)hipDeviceSynchronize();
                (void)hipMemcpy(h.data(), sb.mem.get(), sb.bytes, hipMemcpyDeviceToHost);
                unsigned long long pr[7] = {};
                unsigned blocks = 0;
                const size_t stride = hip_detail::DEFER_WAVE_BYTES / 8;
                for (size_t b = 0; b + 8 <= h.size(); b += stride)
                    if (h[b + 7] == hip_detail::DEFER_PROF_MAGIC) { ++blocks; for (int k = 0; k < 7; ++k) pr[k] += h[b + k]; }
                printf("{\"defer_prof\":{\"blocks\":%u,\"record\":%llu,\"trace\":%llu,\"replay\":%llu,\"tiles\":%llu,"
                       "\"pool_rays\":%llu,\"trace_iterations\":%llu,\"busy_lanes\":%llu}}\n",
                       blocks, pr[0], pr[1], pr[2], pr[3], pr[4], pr[5], pr[6]);
            }
#endif
            fflush(stdout);
        }
        else if (mode == "frames")
        {
            // frames in flight with a user kernel: three cameras (the eye raised twice) in one frames()
            // launch equal their own frame() calls with frame numbers frame_num + f
            const unsigned frame_num = argc > 6 ? unsigned(strtoul(argv[6], nullptr, 10)) : 5u;
            hip_bvh_ref const* begin = one.r;
            hip_bvh_ref const* end = one.r + one.n;
            auto k = [=] __device__ (ray r, random_sampler<float>& samp) -> result_record<float>
            {
                result_record<float> result;
                result.color = vec4(0.1f, 0.2f, 0.3f, 1.0f);
                auto hr = closest_hit(r, begin, end);
                result.hit = hr.hit;
                if (hr.hit)
                {
                    result.depth = hr.t;
                    hr.isect_pos = r.ori + r.dir * hr.t;
                    float clr = 1.0f;
                    vec3 n = get_normal(dnormals, hr);
                    vec3 u, v, w = n;
                    make_orthonormal_basis(u, v, w);
                    for (int i = 0; i < 8; ++i)
                    {
                        auto sp = cosine_sample_hemisphere(samp.next(), samp.next());
                        auto dir = normalize(sp.x * u + sp.y * v + sp.z * w);
                        ray ao(hr.isect_pos + dir * 1E-3f, dir);
                        if (any_hit(ao, begin, end, 0.1f).hit) clr = clr - 1.0f / 8;
                    }
                    result.color = vec4(clr, clr, float(hr.prim_id), 1.0f);
                }
                return result;
            };
            // [nframes]: frames per launch (default 3), the eye raised by 0.1 per frame
            const size_t NF = argc > 7 ? size_t(strtoul(argv[7], nullptr, 10)) : 3u;
            std::vector<camera> cams(NF, cam);
            for (size_t f = 1; f < NF; ++f)
                cams[f].look_at(vec3(0.0f, 0.9f + 0.1f * float(f), 1.4f), vec3(0.0f), vec3(0.0f, 1.0f, 0.0f));
            hip_buffer_rt<PF_RGBA32F, PF_UNSPECIFIED> rt3;
            rt3.resize(W, unsigned(NF) * H);
            sched.frames(k, cams, rt3, frame_num);
            const size_t n = size_t(W) * H;
            std::vector<float> c3(4 * NF * n), t3(NF * n), c1(4 * n), t1(n);
            rt3.download(c3.data(), nullptr, t3.data());
            bool ok = true, distinct = false;
            for (size_t f = 0; f < NF; ++f)
            {
                auto sp = make_sched_params(pixel_sampler::uniform_type{}, cams[f], rt);
                sched.frame(k, sp, frame_num + unsigned(f));
                rt.download(c1.data(), nullptr, t1.data());
                ok = ok && std::memcmp(c1.data(), c3.data() + 4 * f * n, 16 * n) == 0
                        && std::memcmp(t1.data(), t3.data() + f * n, 4 * n) == 0;
                if (f > 0) distinct = distinct || std::memcmp(c3.data(), c3.data() + 4 * f * n, 16 * n) != 0;
            }
            printf("{\"mode\":\"frames\",\"frames_ok\":%s,\"distinct\":%s}\n", ok ? "true" : "false",
                   distinct ? "true" : "false");
            return ok && distinct ? 0 : 1;
        }
        else if (mode == "mask")
        {
            if (argc < 8) return 2;
            const int n = atoi(argv[7]);
            std::vector<uint8_t> mask(size_t(n) * n);
            FILE* f = fopen(argv[6], "rb");
            if (!f || fread(mask.data(), 1, mask.size(), f) != mask.size()) return 3;
            fclose(f);
            byte_mask_intersector isect;
            isect.tex_coords = dtc;
            isect.mask = to_device(mask);
            isect.w = n;
            isect.h = n;
            sched.frame(ao_kernel(one, dnormals, isect, W, 0u), sparams);
        }
        else if (mode == "isect")
        {
            // the mask intersector handed over in the sched params (make_sched_params(sampler, cam,
            // rt, isect), scheduler.h:177-193): the kernel is called as kernel(isect, r, x, y)
            if (argc < 8) return 2;
            const int n = atoi(argv[7]);
            std::vector<uint8_t> mask(size_t(n) * n);
            FILE* f = fopen(argv[6], "rb");
            if (!f || fread(mask.data(), 1, mask.size(), f) != mask.size()) return 3;
            fclose(f);
            byte_mask_intersector isect;
            isect.tex_coords = dtc;
            isect.mask = to_device(mask);
            isect.w = n;
            isect.h = n;
            auto isparams = make_sched_params(pixel_sampler::uniform_type{}, cam, rt, isect);
            sched.frame(ao_kernel_isect(one, dnormals, W, 0u), isparams);
        }
        else if (mode == "sampler")
        {
            // make_sched_params(pixel_sampler::<kind>{}, cam, rt) with a user kernel, frame `frame`, onto a
            // target cleared to (0.25, 0.5, 0.75, 1): colour + the last sample's prim id
            if (argc < 8) return 2;
            const std::string kind = argv[6];
            const unsigned frame_num = unsigned(strtoul(argv[7], nullptr, 10));
            std::vector<uint32_t> hp(size_t(W) * H, 0xFFFFFFFFu);
            uint32_t* dpid = to_device(hp);
            auto k = sampler_kernel(one, dnormals, dpid, W, frame_num);
            rt.clear_color_buffer(vec4(0.25f, 0.5f, 0.75f, 1.0f));
            // optional argv[8]: view and projection matrix (32 floats, column-major) -- the camera
            // matrices form make_sched_params(sampler, view, proj, rt) (scheduler.h:197-212)
            const bool mats = argc > 8;
            mat4 view, proj;
            if (mats)
            {
                float m[32];
                FILE* f = fopen(argv[8], "rb");
                if (!f || fread(m, 4, 32, f) != 32) return 3;
                fclose(f);
                view = mat4(m);
                proj = mat4(m + 16);
            }
            auto run = [&](auto ps)
            {
                if (mats) sched.frame(k, make_sched_params(ps, view, proj, rt), frame_num);
                else sched.frame(k, make_sched_params(ps, cam, rt), frame_num);
            };
            if (kind == "jittered") run(pixel_sampler::jittered_type{});
            else if (kind == "jittered_blend") run(pixel_sampler::jittered_blend_type{});
            else if (kind == "ssaa2") run(pixel_sampler::ssaa_type<2>{});
            else if (kind == "ssaa4") run(pixel_sampler::ssaa_type<4>{});
            else if (kind == "ssaa8") run(pixel_sampler::ssaa_type<8>{});
            else run(pixel_sampler::uniform_type{});
            if (hipMemcpy(hp.data(), dpid, hp.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return 4;
            write_file(outdir + "/sampler_prim_id.bin", hp.data(), hp.size() * 4);
        }
        else if (mode == "list")
        {
            // the harness's list mode: the triangles split by prim_id parity into two BVHs, closest_hit
            // / any_hit over the list of both, a scissor box, frame number `frame`
            if (argc < 11) return 2;
            for (int k = 0; k < 4; ++k) box[k] = atoi(argv[6 + k]);
            const unsigned frame_num = unsigned(strtoul(argv[10], nullptr, 10));
            std::vector<tri_t> part[2];
            for (auto const& t : tris) part[t.prim_id % 2u].push_back(t);
            auto h0 = build<index_bvh<tri_t>>(part[0].data(), part[0].size());
            auto h1 = build<index_bvh<tri_t>>(part[1].data(), part[1].size());
            hip_index_bvh<tri_t> d0(h0), d1(h1);
            const ref_list two{ to_device(std::vector<hip_bvh_ref>{ checked_ref(d0.ref()), checked_ref(d1.ref()) }), 2u };
            sparams.scissor_box = recti(box[0], box[1], box[2], box[3]);   // cuda_sched.inl:71 reading
            rt.clear_color_buffer();
            sched.frame(ao_kernel(two, dnormals, default_intersector{}, W, frame_num), sparams, frame_num);
        }
        else if (mode == "divbvh")
        {
            // lanes of one wave walking DIFFERENT BVHs in the same closest_hit / any_hit call (the BVH
            // chosen per pixel, (x ^ y) & 1, of the triangles split by prim_id parity) against the same
            // choice made after wave-uniform calls on both BVHs: equal bit for bit
            const unsigned frame_num = argc > 6 ? unsigned(strtoul(argv[6], nullptr, 10)) : 0u;
            std::vector<tri_t> part[2];
            for (auto const& t : tris) part[t.prim_id % 2u].push_back(t);
            auto h0 = build<index_bvh<tri_t>>(part[0].data(), part[0].size());
            auto h1 = build<index_bvh<tri_t>>(part[1].data(), part[1].size());
            hip_index_bvh<tri_t> d0(h0), d1(h1);
            hip_bvh_ref const* two = to_device(std::vector<hip_bvh_ref>{ checked_ref(d0.ref()), checked_ref(d1.ref()) });
            auto body = [=] __device__ (ray r, unsigned x, unsigned y, bool divergent) -> result_record<float>
            {
                const unsigned sel = (x ^ y) & 1u;
                auto pick = [&](auto&& call) {
                    if (divergent) return call(two + sel);
                    auto a = call(two);
                    auto b = call(two + 1);
                    return sel ? b : a;
                };
                result_record<float> result;
                result.color = vec4(__uint_as_float(0xFFFFFFFFu), -1.0f, 0.0f, 1.0f);
                auto hr = pick([&](hip_bvh_ref const* p) { return closest_hit(r, p, p + 1); });
                result.hit = hr.hit;
                if (!hr.hit) return result;
                hr.isect_pos = r.ori + r.dir * hr.t;
                vec3 n = get_normal(dnormals, hr);
                vec3 uu, vv, w = n;
                make_orthonormal_basis(uu, vv, w);
                unsigned mask = 0, recs = 0x811C9DC5u;
                for (unsigned smp = 0; smp < 8; ++smp)
                {
                    vec3 s = hip_ao_sample(y * W + x, smp, frame_num);
                    auto dir = normalize(s.x * uu + s.y * vv + s.z * w);
                    ray ao(hr.isect_pos + dir * 1E-3f, dir);
                    auto ar = pick([&](hip_bvh_ref const* p) { return any_hit(ao, p, p + 1, 0.1f); });
                    if (ar.hit) mask |= 1u << smp;
                    recs = (recs ^ (ar.hit ? unsigned(ar.prim_id) : 0xFFFFFFFFu)) * 16777619u;
                }
                // x, y, z: the primary record and the AO hit / miss bits; w: the any_hit records
                result.color = vec4(__uint_as_float(unsigned(hr.prim_id)), hr.t, __uint_as_float(mask), __uint_as_float(recs));
                return result;
            };
            std::vector<float> a(4 * size_t(W) * H), b(4 * size_t(W) * H);
            sched.frame([=] __device__ (ray r, unsigned x, unsigned y) { return body(r, x, y, true); }, sparams, frame_num);
            rt.download(a.data());
            sched.frame([=] __device__ (ray r, unsigned x, unsigned y) { return body(r, x, y, false); }, sparams, frame_num);
            rt.download(b.data());
            size_t hits = 0;
            bool same_hits = true;
            for (size_t p = 0; p < size_t(W) * H; ++p)
            {
                uint32_t bits;
                memcpy(&bits, &b[4 * p], 4);
                hits += bits != 0xFFFFFFFFu;
                same_hits = same_hits && std::memcmp(&a[4 * p], &b[4 * p], 12) == 0;
            }
            const bool same = std::memcmp(a.data(), b.data(), a.size() * 4) == 0;
            printf("{\"mode\":\"divbvh\",\"same\":%s,\"same_hits\":%s,\"hits\":%zu}\n", same ? "true" : "false",
                   same_hits ? "true" : "false", hits);
            return same_hits && hits > 0 ? 0 : 1;
        }
        else if (mode == "heart")
        {
            heart_intersector isect;
            isect.tex_coords = dtc;
            sched.frame(primary_kernel(ref, isect), sparams);
        }
        else
            return 2;

        const size_t npx = size_t(W) * H;
        std::vector<float> out(4 * npx);
        rt.download(out.data());
        if (mode == "sampler")
        {
            write_file(outdir + "/sampler_color.bin", out.data(), out.size() * 4);    // RGBA32F as rendered
            return 0;
        }
        write_outputs(outdir, mode, W, H, out, box);
    }
    catch (hip_error const& e)
    {
        return report_hip_error(e);
    }
    catch (std::exception const& e)
    {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
