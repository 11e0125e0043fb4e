// tests/golden/multi_volume_ref.cpp -- fixture generator for the multi-volume kernel (vrh_render_multi_volume,
// vrh_multi_volume_render_host).
//
// States, in this project's own words, what the functor of the reference's multi-volume example computes
// (src/examples/multi_volume/main.cpp:410-567) for scalar float rays, and evaluates it on the CPU with the
// reference's own tex3D, tex1D, intersect(ray, aabb), matrix<4, 4>, inverse(), plastic<float>::shade, shade_record
// and point_light, called from the reference's headers (nothing of the reference is copied into this
// repository), over a file written by make_multi_volume_golden.py:
//
//     multi_volume_ref <in.bin> <out.bin>
//
// in.bin: the `frame_header` below; then per volume a `volume_header`, its voxels and its transfer function.
// The model transform of a volume is the product translation * rotation(axis, angle) * scaling, as the example
// places its volumes, inverted with the reference's inverse().  Texel storage is guarded as in volume_ref.cpp
// (guard 0: zeros, guard 1: the format's largest value), so that a read outside an array shows as a difference
// between the two runs.  The constants arrive as data.  For the example's own values (step 0.007f, threshold
// 0.1f, gradient offset 0.01f, the double 0.999, coordinates sign (1, -1, -1), offset 1, extent 2) the general
// expressions below are the example's float operations: 1 * p and -1 * p are exact.
//
// What is computed per ray (the multi-volume kernel, has the derivation):
//   - every volume clips the ray, taken into its space by its inverse transform (direction not renormalised), against
//     its box; the march covers [earliest entry, latest exit) over the boxes that were hit
//   - at parameter t every volume whose own interval holds t is sampled at its volume-space position, classified,
//     lit where the classified alpha reaches the threshold and the central difference is not 0, weighted by alpha
//     and added to the step's sum; the sum is composited under what the ray has gathered
//   - the ray stops once its alpha reaches the cutoff
//
// out.bin: per volume the 16 floats of the inverse transform; per pixel the colour (4 floats), then per pixel
// hit (u32), tmin (float), steps (u32); then u64 counters: total steps, steps inside two or more volumes, steps
// inside none, shaded samples, samples with alpha >= shade_alpha and a zero gradient, rays ended by the cutoff.
//
// powf: defined here (built with -fno-builtin-powf) and forwarded to the C library's, as in pathtrace_ref.cpp;
// header.pow_shift = +1 / -1 moves every result one float up / down.
#include <visionaray/math/math.h>
#include <visionaray/texture/texture.h>
#include <visionaray/material.h>
#include <visionaray/point_light.h>
#include <visionaray/shade_record.h>

#include <dlfcn.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

using namespace visionaray;

static int g_pow_shift = 0;

extern "C" float powf(float x, float y)
{
    typedef float (*fn_t)(float, float);
    static fn_t real = (fn_t)dlsym(RTLD_NEXT, "powf");
    float r = real(x, y);
    if (g_pow_shift == 0 || y == 0.0f || x == 1.0f || r == 0.0f || !std::isfinite(r)) return r;
    return nextafterf(r, g_pow_shift > 0 ? INFINITY : -INFINITY);
}

struct frame_header
{
    uint32_t magic;           // 0x4D564F4C
    uint32_t W, H, num_volumes, guard, example;      // `example` marks the case for the script; nothing here reads it
    int32_t pow_shift;
    uint32_t pad;
    float dt, shade_alpha, delta, padf;
    double cutoff;
    float light_pos[3], light_cl[3], light_kl, light_att[3];
    float eye[3], cam_u[3], cam_v[3], cam_w[3];
};

struct volume_header
{
    uint32_t vw, vh, vd, format, filter, address[3];
    uint32_t tf_size, tf_filter, tf_address, pad;
    float box_min[3], box_max[3], sign[3], offset[3], extent[3];
    float axis[3], angle, scaling[3], translation[3];
    float ca[3], ka, cd[3], kd, cs[3], ks, exp;
};

static float guard_float(uint32_t g) { return g ? 3.0e38f : 0.0f; }

static vec3 v3(const float f[3]) { return vec3(f[0], f[1], f[2]); }

// one volume of any of the three texel types behind one sampling interface
struct any_volume
{
    uint32_t format = 0;
    std::vector<uint8_t> store;
    size_t pad_bytes = 0;
    texture_ref<unorm<8>, 3> t8;
    texture_ref<unorm<16>, 3> t16;
    texture_ref<float, 3> t32;

    template <typename T>
    static void setup(texture_ref<T, 3>& t, const void* data, const volume_header& h)
    {
        t = texture_ref<T, 3>(h.vw, h.vh, h.vd);
        t.reset(reinterpret_cast<T const*>(data));
        t.set_filter_mode(h.filter == 0 ? Nearest : Linear);
        for (int a = 0; a < 3; ++a) t.set_address_mode(a, tex_address_mode(h.address[a]));
    }

    bool read(FILE* in, const volume_header& h, uint32_t guard)
    {
        format = h.format;
        const size_t b = format == 0 ? 1 : format == 1 ? 2 : 4;
        const size_t n = size_t(h.vw) * h.vh * h.vd, pad = 2 * size_t(h.vw) * h.vh + 2 * size_t(h.vw) + 8;
        pad_bytes = pad * b;
        store.assign((2 * pad + n) * b, guard ? 0xFF : 0x00);
        if (format == 2)
        {
            const float g = guard_float(guard);
            for (size_t i = 0; i < 2 * pad + n; ++i) memcpy(store.data() + 4 * i, &g, 4);
        }
        if (fread(store.data() + pad_bytes, b, n, in) != n) return false;
        const void* data = store.data() + pad_bytes;
        if (format == 0) setup(t8, data, h);
        else if (format == 1) setup(t16, data, h);
        else setup(t32, data, h);
        return true;
    }

    float sample(vec3 const& c) const
    {
        return format == 0 ? float(tex3D(t8, c)) : format == 1 ? float(tex3D(t16, c)) : tex3D(t32, c);
    }
};

struct any_transfunc
{
    std::vector<float> store;
    texture_ref<vec4, 1> t;
    bool read(FILE* in, const volume_header& h, uint32_t guard)
    {
        store.assign((size_t(h.tf_size) + 16) * 4, guard_float(guard));
        if (fread(store.data() + 32, 16, h.tf_size, in) != h.tf_size) return false;
        t = texture_ref<vec4, 1>(h.tf_size);
        t.reset(reinterpret_cast<vec4 const*>(store.data() + 32));
        t.set_filter_mode(h.tf_filter == 0 ? Nearest : Linear);
        t.set_address_mode(tex_address_mode(h.tf_address));
        return true;
    }
};

// everything one volume of the frame brings along
struct placed_volume
{
    volume_header head;
    any_volume voxels;
    any_transfunc classify;
    mat4 to_local;            // inverse(translation * rotation * scaling)
    aabb box;
    plastic<float> surface;

    // (to_local * (p, w)).xyz(): w = 1 moves a point, w = 0 a direction
    vec3 local(vec3 const& p, float w) const { return (to_local * vec4(p, w)).xyz(); }

    // the texture coordinate of a volume-space point, per axis (sign * p + offset) / extent
    vec3 coordinate(vec3 const& p) const
    {
        return vec3((head.sign[0] * p.x + head.offset[0]) / head.extent[0], (head.sign[1] * p.y + head.offset[1]) / head.extent[1],
                    (head.sign[2] * p.z + head.offset[2]) / head.extent[2]);
    }

    // Central difference of the voxel field at coordinate c with offset d.  Along x it is the sample ahead minus
    // the sample behind; along y and z the sample behind minus the sample ahead (the texture's y and z run
    // against the volume's).  The shifted coordinate is c -+ (an offset vector that is d on one axis, 0 elsewhere).
    vec3 difference(vec3 const& c, float d) const
    {
        vec3 g;
        for (int axis = 0; axis < 3; ++axis)
        {
            vec3 shift(0.0f, 0.0f, 0.0f);
            shift[axis] = d;
            const float behind = voxels.sample(c - shift), ahead = voxels.sample(c + shift);
            g[axis] = axis == 0 ? ahead - behind : behind - ahead;
        }
        return g;
    }
};

struct ray_interval { float enter, leave; };

struct tallies
{
    uint64_t steps = 0, steps_in_several = 0, steps_in_none = 0, lit = 0, flat = 0, cut_rays = 0;
};

struct pixel_result { vec4 gathered; bool hit; float first; uint32_t steps; };

// One volume's contribution at the world-space point `world` of a ray with direction `dir`: classified, lit where
// it is opaque enough and has a gradient, and weighted by its alpha.
static vec4 contribution(placed_volume const& v, frame_header const& h, point_light<float> const& lamp, vec3 const& world,
                         vec3 const& dir, tallies& count)
{
    const vec3 p = v.local(world, 1.0f);
    const vec3 c = v.coordinate(p);
    vec4 rgba = tex1D(v.classify.t, v.voxels.sample(c));
    if (rgba.w >= h.shade_alpha)
    {
        const vec3 g = v.difference(c, h.delta);
        if (length(g) != 0.0f)
        {
            // what the material is asked: the point in the volume's space, the normalised difference as the normal, the
            // way back along the world-space ray, and the lamp's volume-space position vector as the direction to it
            shade_record<point_light<float>, float> ask;
            ask.light = lamp;
            ask.light_dir = normalize(v.local(vec3(lamp.position()), 1.0f));
            ask.view_dir = -dir;
            ask.normal = normalize(g);
            ask.isect_pos = p;
            const vec3 lit = to_rgb(v.surface.shade(ask));
            rgba.xyz() = rgba.xyz() * lit;
            ++count.lit;
        }
        else
            ++count.flat;
    }
    rgba.xyz() *= rgba.w;
    return rgba;
}

static pixel_result march(std::vector<std::unique_ptr<placed_volume>> const& scene, frame_header const& h,
                          point_light<float> const& lamp, basic_ray<float> const& ray, tallies& count)
{
    // where the ray is inside each box, and the span of the boxes it hits
    std::vector<ray_interval> inside(scene.size());
    float first = numeric_limits<float>::max(), last = -numeric_limits<float>::max();
    for (size_t i = 0; i < scene.size(); ++i)
    {
        basic_ray<float> local;
        local.ori = scene[i]->local(ray.ori, 1.0f);
        local.dir = scene[i]->local(ray.dir, 0.0f);
        const auto clip = intersect(local, scene[i]->box);
        inside[i] = { clip.tnear, clip.tfar };
        if (clip.hit && clip.tnear < first) first = clip.tnear;
        if (clip.hit && clip.tfar > last) last = clip.tfar;
    }

    pixel_result px;
    px.gathered = vec4(0.0f);
    px.steps = 0;
    px.first = first;
    px.hit = last > first;
    for (float t = first; t < last; t += h.dt)
    {
        ++px.steps;
        const vec3 world = ray.ori + ray.dir * t;
        vec4 sum(0.0f);
        unsigned holding = 0;
        for (size_t i = 0; i < scene.size(); ++i)
        {
            if (!(t >= inside[i].enter && t < inside[i].leave)) continue;
            ++holding;
            sum += contribution(*scene[i], h, lamp, world, ray.dir, count);
        }
        count.steps_in_several += holding >= 2 ? 1 : 0;
        count.steps_in_none += holding == 0 ? 1 : 0;
        px.gathered += sum * (1.0f - px.gathered.w);
        if (px.gathered.w >= h.cutoff)           // a float against the double, as the example compares
        {
            ++count.cut_rays;
            break;
        }
    }
    count.steps += px.steps;
    return px;
}

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: multi_volume_ref <in.bin> <out.bin>\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    frame_header h;
    if (fread(&h, sizeof(h), 1, in) != 1 || h.magic != 0x4D564F4Cu || h.num_volumes < 1 || h.num_volumes > 32) return 3;
    g_pow_shift = h.pow_shift;

    std::vector<std::unique_ptr<placed_volume>> scene;
    for (uint32_t i = 0; i < h.num_volumes; ++i)
    {
        scene.emplace_back(new placed_volume);
        placed_volume& v = *scene.back();
        if (fread(&v.head, sizeof(volume_header), 1, in) != 1) return 3;
        if (!v.voxels.read(in, v.head, h.guard) || !v.classify.read(in, v.head, h.guard)) return 3;
        const mat4 turn = rotate(mat4::identity(), v3(v.head.axis), v.head.angle);
        const mat4 size = scale(mat4::identity(), v3(v.head.scaling));
        const mat4 move = translate(mat4::identity(), v3(v.head.translation));
        v.to_local = inverse(move * turn * size);
        v.box = aabb(v3(v.head.box_min), v3(v.head.box_max));
        v.surface.set_ca(from_rgb(v3(v.head.ca)));
        v.surface.set_ka(v.head.ka);
        v.surface.set_cd(from_rgb(v3(v.head.cd)));
        v.surface.set_kd(v.head.kd);
        v.surface.set_cs(from_rgb(v3(v.head.cs)));
        v.surface.set_ks(v.head.ks);
        v.surface.set_specular_exp(v.head.exp);
        if (fwrite(v.to_local.data(), 4, 16, out) != 16) return 4;
    }
    point_light<float> lamp;
    lamp.set_position(v3(h.light_pos));
    lamp.set_cl(v3(h.light_cl));
    lamp.set_kl(h.light_kl);
    lamp.set_constant_attenuation(h.light_att[0]);
    lamp.set_linear_attenuation(h.light_att[1]);
    lamp.set_quadratic_attenuation(h.light_att[2]);

    const vec3 eye = v3(h.eye), cam_u = v3(h.cam_u), cam_v = v3(h.cam_v), cam_w = v3(h.cam_w);
    const size_t npx = size_t(h.W) * h.H;
    std::vector<float> color(npx * 4), tmins(npx);
    std::vector<uint32_t> hits(npx), steps(npx);
    tallies count;
    for (uint32_t y = 0; y < h.H; ++y)
        for (uint32_t x = 0; x < h.W; ++x)
        {
            // the primary ray of the pinhole camera (sched_common.h:130-150), uniform pixel sampler
            const float pu = 2.0f * (float(x) + 0.5f) / float(h.W) - 1.0f;
            const float pv = 2.0f * (float(y) + 0.5f) / float(h.H) - 1.0f;
            basic_ray<float> ray;
            ray.ori = eye;
            ray.dir = normalize(cam_u * pu + cam_v * pv + cam_w);
            const pixel_result px = march(scene, h, lamp, ray, count);
            const size_t o = size_t(y) * h.W + x;
            color[4 * o] = px.gathered.x; color[4 * o + 1] = px.gathered.y; color[4 * o + 2] = px.gathered.z; color[4 * o + 3] = px.gathered.w;
            hits[o] = px.hit ? 1u : 0u;
            tmins[o] = px.first;
            steps[o] = px.steps;
        }
    const uint64_t counters[6] = { count.steps, count.steps_in_several, count.steps_in_none, count.lit, count.flat, count.cut_rays };
    if (fwrite(color.data(), 16, npx, out) != npx || fwrite(hits.data(), 4, npx, out) != npx
        || fwrite(tmins.data(), 4, npx, out) != npx || fwrite(steps.data(), 4, npx, out) != npx
        || fwrite(counters, 8, 6, out) != 6)
        return 4;
    fclose(in);
    fclose(out);
    return 0;
}
