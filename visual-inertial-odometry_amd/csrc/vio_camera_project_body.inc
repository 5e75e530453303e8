// vio_camera_project_body.inc — k_camera_project, the kernel of include/vio_camera_project.h (DESIGN.md section 37), compiled into
// libvio_camera_hip alone (vio_camera.hip includes it behind vio_reject_body.inc, whose NT it uses).  The including file has included
// vio_camera_project_math.h and has contraction off.
// A thread per point, items by offset, as k_reject_lift is laid out: blockIdx.y is the item, blockIdx.x the item's block of NT points;
// a block beyond the item's points returns whole.  The thread reads its point's three doubles, the item's entry of the projection
// table (uniform over the workgroup), and writes the pixel's two doubles and the flag byte at the item's offset.  No LDS, no barrier,
// no atomics; every index is below the call's point total, which sized the buffers.
struct ProjItem {
    int32_t n, slot;
    int64_t o_pt;       // the item's first point in the staged points and in the outputs
};

struct ProjArgs {
    const ProjItem *items;
    const double *pts;      // [points][3]
    double *pix;            // [points][2]
    uint8_t *flags;         // [points]
    const CamProj *cams;    // [VIO_CAMERA_MAX_SLOTS]
    int32_t count, pad;
};

__global__ __launch_bounds__(NT) void k_camera_project(ProjArgs a) {
    const int item = blockIdx.y;
    if (item >= a.count) return;
    const ProjItem &D = a.items[item];
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= D.n || D.slot < 0 || D.slot >= VIO_CAMERA_MAX_SLOTS) return;
    const int64_t at = D.o_pt + i;
    const double *P = a.pts + 3 * at;
    double u, v;
    const int flag = cam_project(a.cams[D.slot], P[0], P[1], P[2], u, v);
    a.pix[2 * at] = u; a.pix[2 * at + 1] = v;
    a.flags[at] = (uint8_t)flag;
}
