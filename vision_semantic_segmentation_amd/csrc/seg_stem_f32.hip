// The fp32 plan's stem with the node's pre-processing in its loader (vision_semantic_segmentation_node.py:83-98: BGR->RGB,
// cv2.undistort, INTER_AREA by an integer factor): the counterpart of k_stem_mfma<PRE> for the plan that has no 16-bit stem.
//
// A workgroup owns an 8 x 32 tile of stem outputs.  It first fills LDS with the NORMALISED fp32 input tile, halo included
// (21 x 69 pixels x 3 channels, 17 KB): every tile pixel is preprocessed_rgb() of seg_preprocess.h -- the function k_preprocess
// applies -- computed once, then normalised with k_stem's own expression; pixels outside the network input are 0 (padding applies
// to the normalised image, and a raw frame whose size leaves a remainder is padded, not pre-processed, beyond H x W).  Then each
// lane computes one output pixel x 64 channels with k_stem's fmaf chain: bias first, taps in [ky][kx][ci] order, the same
// [ky][kx][ci][co] weights (wave-uniform addresses: scalar loads, v_fmac with an SGPR operand), ReLU, fp32 store.  The result is
// therefore the same bits as avl_preprocess_image followed by the plain fp32 stem, without the RGB frame in between.
// A batch of raw frames (avl_seg_op.raw_batch): image blockIdx.z, each with a camera block of its own, as in k_stem_mfma<PRE>.
#include "seg_types.h"
#include "seg_preprocess.h"

namespace avl {
namespace {

constexpr int F_TH = 8, F_TW = 32;                               // outputs per workgroup: one per lane
constexpr int F_IH = 2 * F_TH + 5, F_IW = 2 * F_TW + 5;         // 21 x 69 input pixels
constexpr int F_ROW = F_IW * 3;                                 // floats per LDS row

__global__ void __launch_bounds__(256) k_stem_pre_f32(const unsigned char* __restrict__ bgr0, int srcH, int srcW, int factor,
                                                     const PreCamera* __restrict__ cam_dev, int H, int W,
                                                     const float* __restrict__ w, const float* __restrict__ bias,
                                                     float* __restrict__ out0, int OH, int OW, int out_ld, int tiles_x) {
    __shared__ float tile[F_IH * F_ROW];
    // batch of raw frames (raw_batch): frame blockIdx.z, its output rows and ITS camera block (AVL_STEM_CAMERA_BYTES apart)
    const unsigned char* __restrict__ bgr = image_base(bgr0, (long long)srcH * srcW, 3);
    float* __restrict__ out = image_base(out0, (long long)OH * OW, out_ld);
    cam_dev = reinterpret_cast<const PreCamera*>(reinterpret_cast<const char*>(cam_dev) + (long long)blockIdx.z * AVL_STEM_CAMERA_BYTES);
    const int tid = threadIdx.x;
    const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
    const int oy0 = ty * F_TH, ox0 = tx * F_TW;
    const int iy0 = oy0 * 2 - 3, ix0 = ox0 * 2 - 3;
    const float mean[3] = {0.485f, 0.456f, 0.406f}, stdv[3] = {0.229f, 0.224f, 0.225f};
    const PreCamera cam = *cam_dev;
    for (int i = tid; i < F_IH * F_IW; i += 256) {
        const int ly = i / F_IW, lx = i - ly * F_IW;
        const int iy = iy0 + ly, ix = ix0 + lx;
        float* t = tile + ly * F_ROW + lx * 3;
        if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
            int rgb[3];
            preprocessed_rgb(bgr, srcH, srcW, cam, factor, ix, iy, rgb);
#pragma unroll
            for (int c = 0; c < 3; ++c) t[c] = ((float)rgb[c] / 255.0f - mean[c]) / stdv[c];
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) t[c] = 0.0f;
        }
    }
    __syncthreads();

    const int sy = tid / F_TW, sx = tid % F_TW;
    float acc[64];
#pragma unroll
    for (int c = 0; c < 64; ++c) acc[c] = bias[c];
    for (int ky = 0; ky < 7; ++ky) {
        const float* row = tile + (sy * 2 + ky) * F_ROW + sx * 6;
        for (int kx = 0; kx < 7; ++kx) {
#pragma unroll
            for (int ci = 0; ci < 3; ++ci) {
                const float x = row[kx * 3 + ci];
                const float* wr = w + ((ky * 7 + kx) * 3 + ci) * 64;
#pragma unroll
                for (int c = 0; c < 64; ++c) acc[c] = fmaf(x, wr[c], acc[c]);
            }
        }
    }
    const int oy = oy0 + sy, ox = ox0 + sx;
    if (oy < OH && ox < OW) {
        float* op = out + ((long long)oy * OW + ox) * out_ld;
#pragma unroll
        for (int c8 = 0; c8 < 8; ++c8) {
            float v[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = fmaxf(acc[c8 * 8 + i], 0.f);
            Vec8<float>::store(op + c8 * 8, v);
        }
    }
}

}  // namespace

// (validated by validate_conv_op: AVL_F32, w_layout 0, in_rows = batch * src_h * src_w -- batch > 1 only with raw_batch --, in2_ld = src_w,
// integer factor)
int launch_stem_pre_f32(const avl_seg_op& op, hipStream_t s) {
    const int srcW = op.in2_ld, srcH = op.in_rows / op_batch(op) / op.in2_ld, factor = srcW / op.in_w;
    const int tiles_x = (op.out_w + F_TW - 1) / F_TW, tiles_y = (op.out_h + F_TH - 1) / F_TH;
    hipLaunchKernelGGL(k_stem_pre_f32, dim3(tiles_x * tiles_y, 1, op_batch(op)), dim3(256), 0, s, static_cast<const unsigned char*>(op.in), srcH, srcW,
                       factor, static_cast<const PreCamera*>(op.in2), op.in_h, op.in_w, static_cast<const float*>(op.weight), op.bias,
                       static_cast<float*>(op.out), op.out_h, op.out_w, op.out_ld, tiles_x);
    AVL_LAUNCH_CHECK();
    return AVL_OK;
}

}  // namespace avl
