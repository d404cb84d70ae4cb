// model_frame.hpp -- the one thing the dense tracker needs from the volume: a view of the fused model as an RGB-D frame in device memory
// (raycast.hip defines it; odometry.hip's op_tracker_track_model uses it as the source frame of a track).
#pragma once
#include "common.hpp"

namespace op {

// Raycast of `v` at camera-to-world `pose` with `cam` (NULL: the volume's camera), packed as fusion and the tracker read a frame: d_rgb 3 bytes per pixel,
// d_depth float metres (0 = no hit), *d_n_valid = pixels with depth > 0.  All three are DEVICE pointers.  The frames queued on the volume are fused first;
// the kernels are enqueued on the volume's stream (returned in *stream) and NOT waited for.
int volume_render_frame_enqueue(op_volume* v, const op_camera* cam, const float pose[16], unsigned char* d_rgb, float* d_depth, unsigned long long* d_n_valid,
                                hipStream_t* stream);
int volume_device(const op_volume* v);
hipStream_t volume_stream(const op_volume* v);

} // namespace op
