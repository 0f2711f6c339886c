// dmx_zip_host.cpp -- the index of a ZIP archive on the host (include/dmx.h: dmx_zip_index_host): the
// serial walk over the steps of dmx_zip.h, which the device index (dmx_zip_dev.hip) runs a thread
// per position.  Host code only: no device, no HIP.
#include <stdint.h>

#include "../../include/dmx.h"
#include "dmx_zip.h"

static_assert(sizeof(dmx_zip_entry) == 64 && sizeof(dmx_zip_status) == 40, "record layout");

extern "C" int dmx_zip_index_host(const void* zv, uint64_t zbytes, dmx_zip_entry* entries, uint32_t cap,
                                  dmx_zip_status* status) {
    if (!status || (!zv && zbytes) || (!entries && cap)) return -(int)E_INVAL;
    const uint8_t* z = static_cast<const uint8_t*>(zv);
    dmx_zip_status r = {0, 0, 0, 0, 0, 0, 0};
    dmx_zip_tail t;
    dmx_zip_end_parse(z, zbytes, zbytes > DMX_ZIP_MAXZ ? ~0ull : dmx_zip_end_find(z, zbytes), &t);
    r.status = t.status;
    if (!t.status) {
        r.cd_off = t.cd_begin;
        r.cd_len = t.cd_end - t.cd_begin;
        // the chain: exactly nentries headers from cd_begin that end at cd_end
        uint64_t p = t.cd_begin;
        uint32_t n = 0;
        for (; n < t.nentries && p < t.cd_end; n++) {
            const uint32_t len = dmx_zip_cd_step(z, t.cd_end, p);
            if (!len) break;
            p += len;
        }
        if (n != t.nentries || p != t.cd_end) r.status = -(int)E_LEN;
    }
    if (!r.status) {
        uint64_t p = t.cd_begin, sum = 0;
        for (uint32_t i = 0; i < t.nentries; i++) {
            dmx_zip_entry e;
            dmx_zip_finish(z, zbytes, t.concat, p, &e);
            e.out_off = sum;
            sum += dmx_zip_len(&e);
            if (i < cap) entries[i] = e;
            p += dmx_zip_cd_step(z, t.cd_end, p);
        }
        r.nentries = t.nentries;
        r.out_len = sum;
        if (t.nentries > cap) r.status = -(int)E_SZ;
    }
    *status = r;
    return 0;
}
