/* l2o_vgg16_abi.h -- the VGG-16 optimizee on CIFAR-10 (problems.vgg16_cifar10): the part of the C ABI of libl2o_hip.so that was
 * added after ABI v15.  Conventions (error codes, l2o_last_error): l2o_abi.h, which this header includes.  (A header of its
 * own: l2o_abi.h's list of exports is the v15 list.) */
#ifndef L2O_VGG16_ABI_H
#define L2O_VGG16_ABI_H

#include "l2o_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define L2O_PROB_VGG16 10      /* problems.vgg16_cifar10 :637-694, DM/vgg16.py (own entry point: l2o_vgg16_fg) */
#define L2O_VGG16_VARS 28      /* 13 conv layers and the linear layer: weights, biases                         */

/* problems.vgg16_cifar10 (DM/problems.py:637-694, DM/vgg16.py:44-98; DM/util.py:192-197 "vgg16"): NHWC 32x32x3 images ->
 * five blocks of (2, 2, 3, 3, 3) layers of widths channels[0..4], each layer conv 3x3 stride 1 SAME + bias -> ReLU, each
 * block closed by max-pool 2x2 stride 2 (32 -> 16 -> 8 -> 4 -> 2 -> 1) -> flatten (channels[4]) -> linear x10 + bias ->
 * softmax -> mean sparse softmax cross-entropy that takes those PROBABILITIES as its logits (the reference's quirk):
 *   loss = mean_b -log softmax(p_b)[label_b],  p_b = softmax(z_b).
 * No batch norm, no dropout.  The step-granular evaluation only: loss + gradients of one minibatch; the convolutions, their
 * input gradients and their weight gradients are implicit GEMMs on v_mfma_f32_32x32x2_f32 (exact fp32 products, a k-ordered
 * fmaf chain), the weight gradients split over the minibatch with partials summed in a fixed order; no atomics: two calls on
 * the same inputs are bit-identical, and g == NULL (forward only) gives the same loss bits.  No fused unroll.
 * w / g: HOST arrays of L2O_VGG16_VARS device pointers in the reference's variable order
 *   block1_conv1/weights [3,3,3,c0] (HWIO), block1_conv1/biases [c0], block1_conv2/weights [3,3,c0,c0], .../biases, ...,
 *   block5_conv3/weights [3,3,c4,c4], block5_conv3/biases [c4], fc/weights [c4,10], fc/biases [10]
 * (g may be NULL; every entry of every g[k] is written).  batch in [2, 1024] and every channels[i] a multiple of 8 in
 * [8, 512], else L2O_ERR_UNSUPPORTED (l2o_vgg16_scratch_floats: 0).  scratch 16-byte aligned; nothing is kept in it between
 * calls and no entry is read that the call has not written.  Reference width is channels = {64, 128, 256, 512, 512}. */
typedef struct l2o_vgg16 {
  int32_t batch;         /* minibatch size                            */
  int32_t n_data;        /* rows of `images`                          */
  int32_t flags;         /* 0                                         */
  int32_t channels[5];   /* width of the layers of each block         */
  const float* images;   /* device [n_data, 3072] (NHWC 32x32x3)      */
  const int32_t* labels; /* device [n_data]                           */
} l2o_vgg16;
size_t l2o_vgg16_scratch_floats(const l2o_vgg16* net);
int l2o_vgg16_fg(const l2o_vgg16* net, const int32_t* indices /* device [batch] rows of the minibatch */,
                 const float* const* w, float* loss /* device [1] */, float* const* g,
                 float* scratch /* device [l2o_vgg16_scratch_floats] */, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* L2O_VGG16_ABI_H */
