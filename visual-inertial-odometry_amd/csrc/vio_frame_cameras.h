// vio_frame_cameras.h — the slot cameras of libvio_frame_hip (include/vio_frame_camera.h) with no HIP in it:
// which slot has a camera of its own, the table of CamDev the camera kernels read (a slot's own camera, else the handle's PINHOLE
// camera in the same form, else unset), whether that table has changed since it last went up, which of the two sets of kernels a
// read takes, and the lift counts of each slot's last read.  vio_frame.hip uploads the table; tests/cpp/front_cameras_host_main.cpp
// runs a scripted sequence under ASan and UBSan (tests/test_front_cameras_cpu.py).
// The including file has included <cstdint>, <cstring>, ../../include/vio_camera.h, vio_host_base.h, vio_camera_math.h (CamDev,
// cam_device_form: the function libvio_camera_hip derives its table with) and, inside namespace kq, vio_camera_host.h (the check of
// vio_camera_set).
#pragma once

constexpr int FRAME_CAM_SLOTS = 256;            // VIO_FRAME_MAX_SLOTS, VIO_CAMERA_MAX_SLOTS
static_assert(sizeof(CamDev) == 16 + 8 * (2 + VIO_CAMERA_MAX_PARAMS), "a CamDev has no padding: tables are compared as bytes");

// what a read does about its cameras: the handle's camera through the PINHOLE kernels (the path of include/vio_frame_read.h alone),
// the camera table through the general kernels, or nothing (a listed slot has no camera)
enum FrameCamPath { FRAME_CAM_HANDLE = 0, FRAME_CAM_TABLE, FRAME_CAM_MISSING };

// the handle's vio_reject_camera as the PINHOLE vio_camera_model it is
inline vio_camera_model frame_cam_pinhole_model(const vio_reject_camera &c) {
    vio_camera_model m;
    std::memset(&m, 0, sizeof(m));
    m.model = VIO_CAMERA_MODEL_PINHOLE; m.width = c.width; m.height = c.height;
    m.params[0] = c.k1; m.params[1] = c.k2; m.params[2] = c.p1; m.params[3] = c.p2;
    m.params[4] = c.fx; m.params[5] = c.fy; m.params[6] = c.cx; m.params[7] = c.cy;
    return m;
}

struct FrameCameras {
    vio_camera_model model[FRAME_CAM_SLOTS];    // a slot's own camera as it was given (reserved 0); meaningful while own[slot]
    uint8_t own[FRAME_CAM_SLOTS];
    CamDev table[FRAME_CAM_SLOTS];              // what the device's table must hold
    CamDev handle_dev;                          // the handle's camera as a PINHOLE CamDev; set == 0: there is none
    int32_t n_own = 0;
    bool dirty = true;                          // the table differs from the device's (which starts undefined)
    int32_t n_clamped[FRAME_CAM_SLOTS], n_bad[FRAME_CAM_SLOTS];     // of the slot's last read

    FrameCameras() {
        std::memset(model, 0, sizeof(model));
        std::memset(own, 0, sizeof(own));
        std::memset(table, 0, sizeof(table));
        std::memset(&handle_dev, 0, sizeof(handle_dev));
        std::memset(n_clamped, 0, sizeof(n_clamped));
        std::memset(n_bad, 0, sizeof(n_bad));
    }

    static bool slot_ok(int32_t s) { return s >= 0 && s < FRAME_CAM_SLOTS; }

    void put(int32_t slot, const CamDev &d) {
        if (std::memcmp(&table[slot], &d, sizeof(CamDev)) == 0) return;
        table[slot] = d;
        dirty = true;
    }

    // The slot's own camera under vio_camera_set's rules; a refused camera leaves everything as it was.
    vio_status set(ErrText &err, int32_t slot, const vio_camera_model *cam) {
        if (!slot_ok(slot)) return fail(err, VIO_ERR_BAD_ARG, "vio_frame_set_slot_camera: slot %d is outside [0, %d)", slot, FRAME_CAM_SLOTS);
        const vio_status st = kq::cam_check_model(err, cam);
        if (st != VIO_OK) return st;
        model[slot] = *cam;
        model[slot].reserved = 0;
        n_own += own[slot] ? 0 : 1;
        own[slot] = 1;
        put(slot, cam_device_form(*cam));                  // (CamDev has no padding: put compares bytes)
        return VIO_OK;
    }

    // the slot goes back to the handle's camera
    vio_status clear(ErrText &err, int32_t slot) {
        if (!slot_ok(slot)) return fail(err, VIO_ERR_BAD_ARG, "vio_frame_set_slot_camera: slot %d is outside [0, %d)", slot, FRAME_CAM_SLOTS);
        n_own -= own[slot] ? 1 : 0;
        own[slot] = 0;
        put(slot, handle_dev);
        return VIO_OK;
    }

    // the handle's checked camera (vio_frame_set_camera): every slot without its own reads it
    void set_handle_camera(const vio_reject_camera &c) {
        handle_dev = cam_device_form(frame_cam_pinhole_model(c));
        for (int32_t s = 0; s < FRAME_CAM_SLOTS; ++s)
            if (!own[s]) put(s, handle_dev);
    }

    bool has_camera(int32_t slot) const { return slot_ok(slot) && table[slot].set != 0; }

    // The path of a read of `count` listed slots (each inside [0, FRAME_CAM_SLOTS)); FRAME_CAM_MISSING: *bad is the first item whose
    // slot has neither a camera of its own nor the handle's.
    FrameCamPath path(int32_t count, const int32_t *slot, int32_t *bad) const {
        bool any_own = false;
        for (int32_t i = 0; i < count; ++i) {
            if (!has_camera(slot[i])) { *bad = i; return FRAME_CAM_MISSING; }
            any_own = any_own || own[slot[i]] != 0;
        }
        *bad = -1;
        return any_own ? FRAME_CAM_TABLE : FRAME_CAM_HANDLE;
    }

    // the table as the device will have it: true if it has to go up (the caller copies `table` and the flag is down from here on)
    bool take_dirty() {
        const bool d = dirty;
        dirty = false;
        return d;
    }

    void lift_info_set(int32_t slot, int32_t clamped, int32_t bad) {
        if (!slot_ok(slot)) return;
        n_clamped[slot] = clamped; n_bad[slot] = bad;
    }
};
