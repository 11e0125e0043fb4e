// visionaray_amd/csrc/vrh_volobj.h -- the device volume object and what the two volume kernels' entry points
// share (vrh_volume.hip, which defines the functions, and vrh_multi_volume.hip).
#pragma once

#include "vrh_objects.h"
#include "vrh_volhost.h"

struct vrh_volume
{
    vrh_ctx* ctx = nullptr;
    void* voxels = nullptr;
    vrh::dev::rgba_t* entries = nullptr;
    vrh::dev::vol_view vol{};
    vrh::dev::tf_view tf{};
};

namespace vrh {

// Before a volume frame is launched: the context's step counters exist, the frame is ordered after every frame
// issued so far and after a render group's writes into the target, and the previous volume frame's flag has
// been looked at.  VRH_OK, or the error to return.
int volume_frame_begin(vrh_ctx* ctx, vrh_rt* rt);
// behind the frame: the totals for the host, there once the stream has been waited for
int volume_frame_end(vrh_ctx* ctx);

} // namespace vrh
