// fear_train_metrics.h — the training step's telemetry on gfx950: what the reference's `_training_step` does
// on the host after every step (model_training/train/fear_lightning_model.py:66-87) from the step's own output maps, without
// a copy of the maps and without a host synchronisation:
//   decode     FEARBoxCoder.decode (decode_wave of fear_kernels.h: fp32 sigmoid, first maximum, float64 grid)
//   IoU        box_convert(xywh -> xyxy) on both boxes, torchvision.ops.box_iou's diagonal, float64
//   metrics    BoxIoUMetric, TrackingFailureRateMetric (metrics/tracking.py), DatasetAwareMetric (metrics/dataset_aware_metric.py)
// Two launches: one wave per pair writes the pair's IoU; one wave then adds them up in pair-index order (lane d owns dataset d),
// so the sums do not depend on how the first launch was scheduled — no atomics.  feartracker_amd/metrics.py restates the
// arithmetic in numpy (`step_metrics_host`); the per-pair IoUs agree bit for bit.
// Included by fear_train.hip after the training operators.

namespace {

using namespace fear;

struct MetricsArgs {
    const float* cls;           // [B][256] logits
    const float* bbox;          // [B][4][256] l, t, r, b
    const int32_t* gt_box;      // [B][4] x, y, w, h in search-crop pixels
    const int32_t* visible;     // [B]
    const int32_t* dataset_id;  // [B] in [0, D)
    double* iou;                // [B] out: the pair's IoU, -1 for an invisible pair
    double* step;               // [3] out: mean IoU | failure rate | visible pairs
    double* accum;              // [3 + 2 D] in / out: sum of step mean IoUs | sum of step failure rates | steps | D sums | D counts
    int B, D;
};

// torchvision.ops.box_iou of one pair of xywh boxes (boxes.py: box_area, _box_inter_union), every float64 operation rounded on its
// own.  box_convert: x2 = x + w, y2 = y + h.
__device__ __forceinline__ double xywh_iou(double px, double py, double pw, double ph, double gx, double gy, double gw, double gh) {
#pragma clang fp contract(off)
    const double px2 = px + pw, py2 = py + ph, gx2 = gx + gw, gy2 = gy + gh;
    const double area_p = (px2 - px) * (py2 - py);
    const double area_g = (gx2 - gx) * (gy2 - gy);
    const double w = fmax(fmin(px2, gx2) - fmax(px, gx), 0.0);       // (rb - lt).clamp(min=0)
    const double h = fmax(fmin(py2, gy2) - fmax(py, gy), 0.0);
    const double inter = w * h;
    const double uni = area_p + area_g - inter;
    return inter / uni;
}

__global__ __launch_bounds__(64) void metrics_iou_kernel(MetricsArgs a) {
    const int b = blockIdx.x;
    if (a.visible[b] == 0) {                    // (uniform over the wave)
        if (threadIdx.x == 0) a.iou[b] = -1.0;
        return;
    }
    const Decoded d = decode_wave(a.cls + (long)b * 256, a.bbox + (long)b * 1024, FEAR_TP_SCORE, FEAR_TP_SEARCH / FEAR_TP_SCORE,
                                  FEAR_TP_SEARCH);
    if (threadIdx.x != 0) return;
    const int32_t* g = a.gt_box + (long)b * 4;
    a.iou[b] = xywh_iou(d.x0, d.y0, d.w, d.h, (double)g[0], (double)g[1], (double)g[2], (double)g[3]);
}

// One wave.  The IoUs are staged through LDS 256 at a time; every lane then walks them in pair order: all lanes form the same
// batch sum, lane d also the sum and count of dataset d.  A step without a visible pair leaves the accumulators as they are.
__global__ __launch_bounds__(64) void metrics_reduce_kernel(MetricsArgs a) {
#pragma clang fp contract(off)
    __shared__ double s_iou[256];
    __shared__ int s_ds[256];                   // the pair's dataset, -1 for an invisible pair
    const int lane = threadIdx.x;
    double total = 0.0, mine = 0.0;
    long n_vis = 0, n_nonzero = 0, n_mine = 0;
    for (int base = 0; base < a.B; base += 256) {
        const int n = min(256, a.B - base);
        __syncthreads();
        for (int i = lane; i < n; i += 64) {
            s_iou[i] = a.iou[base + i];
            s_ds[i] = a.visible[base + i] != 0 ? a.dataset_id[base + i] : -1;
        }
        __syncthreads();
        for (int i = 0; i < n; ++i) {
            const int ds = s_ds[i];
            if (ds < 0) continue;
            const double v = s_iou[i];
            total = total + v;
            ++n_vis;
            n_nonzero += v != 0.0 ? 1 : 0;          // torch.count_nonzero: a NaN counts
            if (ds == lane) { mine = mine + v; ++n_mine; }
        }
    }
    const double mean = n_vis ? total / (double)n_vis : 0.0;
    const double fail = n_vis ? 1.0 - (double)n_nonzero / (double)n_vis : 0.0;
    if (lane == 0) {
        a.step[0] = mean;
        a.step[1] = fail;
        a.step[2] = (double)n_vis;
        if (n_vis) {
            a.accum[0] = a.accum[0] + mean;
            a.accum[1] = a.accum[1] + fail;
            a.accum[2] = a.accum[2] + 1.0;
        }
    }
    if (lane < a.D && n_mine) {
        a.accum[3 + lane] = a.accum[3 + lane] + mine;
        a.accum[3 + a.D + lane] = a.accum[3 + a.D + lane] + (double)n_mine;
    }
}

}  // namespace

extern "C" {

int fear_train_metrics(const float* cls, const float* bbox, const int32_t* gt_box, const int32_t* visible, const int32_t* dataset_id,
                       int B, int n_datasets, double* iou, double* step3, double* accum, void* stream) {
    if (B < 0 || B > 65535 || n_datasets < 1 || n_datasets > FEAR_METRICS_MAX_DATASETS) return FEAR_TRAIN_ERR_SHAPE;
    if (B == 0) return FEAR_TRAIN_OK;
    if (!cls || !bbox || !gt_box || !visible || !dataset_id || !iou || !step3 || !accum) return FEAR_TRAIN_ERR_NULL;
    const MetricsArgs a{cls, bbox, gt_box, visible, dataset_id, iou, step3, accum, B, n_datasets};
    hipLaunchKernelGGL(metrics_iou_kernel, dim3((unsigned)B), dim3(64), 0, static_cast<hipStream_t>(stream), a);
    hipLaunchKernelGGL(metrics_reduce_kernel, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), a);
    LAUNCH_CHECK();
    return FEAR_TRAIN_OK;
}

}  // extern "C"
