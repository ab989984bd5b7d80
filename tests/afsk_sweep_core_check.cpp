// Host checker for csrc/pm_afsk_sweep.h (tests/test_afsk_sweep_core.py): evaluates the bound E, the matrix-pipe constants, the LDS
// layouts and the launch routes of the certified AFSK sweeps for the cases of a text file and prints every number -- floats as hex --
// one line per case.
//   <n>  then n lines   name m ml mb kb one gmax lpf_abs_sum x_bound tap_dev e_x S tapq_int qabs dlow
//   <g>  then g lines   name kb mb nsweeps  (m ml one) x nsweeps  planned aligned afsk_split
//   <r>  then r lines   name m ml groups tones mb plan_ml own_list afsk_unfused afsk_lpf8 sweep_no_tail
#include <cstdio>
#include <cstring>
#include "pm_afsk_sweep.h"

using namespace pm_sweep;

static void split(const char *tag, int m, int ml, bool one, int mb)
{
    const SweepShape s{m, ml, one};
    const Lpf8Layout Y = lpf8_layout(&s, 1, mb, 0);
    printf(" %s_region0=%d %s_lds=%zu %s_lds_ok=%d %s_off_planes=%zu %s_off_tpl=%zu %s_off_band=%zu %s_off_list=%zu %s_off_max=%zu %s_xw_doubles=%d %s_plane_bytes=%d", tag,
           Y.region0, tag, Y.lds, tag, (int)Y.lds_ok, tag, Y.off_planes, tag, Y.off_tpl, tag, Y.off_band, tag, Y.off_list, tag, Y.off_max, tag, Y.xw_doubles, tag, Y.plane_bytes);
}

int main(int argc, char **argv)
{
    FILE *f = argc == 2 ? fopen(argv[1], "r") : nullptr;
    int n = 0, g = 0;
    if (!f || fscanf(f, "%d", &n) != 1) return 2;
    for (int i = 0; i < n; ++i) {
        char nm[64];
        int m, ml, mb, kb, one, S;
        double gmax, lpf_abs_sum, x_bound, tap_dev, e_x, tapq_int, qabs, dlow;
        if (fscanf(f, "%63s %d %d %d %d %d %lf %lf %lf %lf %lf %d %lf %lf %lf", nm, &m, &ml, &mb, &kb, &one, &gmax, &lpf_abs_sum, &x_bound, &tap_dev, &e_x, &S, &tapq_int,
                   &qabs, &dlow) != 15)
            return 3;
        pm_afsk_tones tn;
        memset(&tn, 0, sizeof(tn));
        tn.tap_dev = tap_dev;
        printf("%s E12=%a E12x=%a E16=%a E16x=%a E0=%a slide12=%a slide16=%a", nm, sweep_bound(m, lpf_abs_sum, gmax, x_bound, &tn, kFuseRun, 0.0),
               sweep_bound(m, lpf_abs_sum, gmax, x_bound, &tn, kFuseRun, e_x), sweep_bound(m, lpf_abs_sum, gmax, x_bound, &tn, kSlideRun, 0.0),
               sweep_bound(m, lpf_abs_sum, gmax, x_bound, &tn, kSlideRun, e_x), sweep_bound(m, lpf_abs_sum, gmax, x_bound, nullptr, kSlideRun, 0.0),
               slide_bound(&tn, m, x_bound, kFuseRun), slide_bound(&tn, m, x_bound));
        const Lpf8Consts Q = lpf8_consts(S, tapq_int, qabs, dlow, gmax, one != 0);
        printf(" S=%d c_tap=%a c_q=%a gfac=%a qabs=%a", Q.S, Q.c_tap, Q.c_q, Q.gfac, Q.qabs);
        split("sp0", m, ml, one != 0, 0);
        split("sp", m, ml, one != 0, mb);
        printf(" runs=%d tail=%zu fuse_region0=%zu fuse_image=%zu fuse_lds=%zu\n", sweep_runs(ml), sweep_tail_doubles(m, ml, mb), fuse_region0(m, ml), fuse_image(ml),
               fuse_lds_bytes(m, ml));
    }
    if (fscanf(f, "%d", &g) != 1) return 4;
    for (int i = 0; i < g; ++i) {
        char nm[64];
        int kb, mb, ns;
        SweepShape s[2];
        if (fscanf(f, "%63s %d %d %d", nm, &kb, &mb, &ns) != 4 || ns < 1 || ns > 2) return 5;
        for (int k = 0; k < ns; ++k) {
            int one = 0;
            if (fscanf(f, "%d %d %d", &s[k].m, &s[k].ml, &one) != 3) return 6;
            s[k].one = one != 0;
        }
        int planned, aligned, split;
        if (fscanf(f, "%d %d %d", &planned, &aligned, &split) != 3) return 7;
        const Lpf8Layout Y = lpf8_layout(s, ns, mb, kb);
        printf("%s takes=%d xs_span=%d mmax=%d aplane=%d xw_doubles=%d plane_bytes=%d region0=%d lds_ok=%d lds=%zu fuses=%d off_planes=%zu off_tpl=%zu off_band=%zu off_list=%zu off_max=%zu\n", nm,
               (int)group_fuses(Y, kb, planned != 0, aligned != 0, SweepSwitches{false, false, false, split != 0}), Y.xs_span, Y.mmax, Y.aplane, Y.xw_doubles, Y.plane_bytes, Y.region0, (int)Y.lds_ok, Y.lds, (int)Y.fuses, Y.off_planes, Y.off_tpl, Y.off_band, Y.off_list, Y.off_max);
    }
    int r = 0;
    if (fscanf(f, "%d", &r) != 1) return 8;
    for (int i = 0; i < r; ++i) {
        char nm[64];
        int m, ml, groups, tones, mb, plan_ml, own_list, unfused, lpf8, no_tail;
        if (fscanf(f, "%63s %d %d %d %d %d %d %d %d %d %d", nm, &m, &ml, &groups, &tones, &mb, &plan_ml, &own_list, &unfused, &lpf8, &no_tail) != 11) return 9;
        const SweepRouting R = sweep_route(m, ml, groups, tones != 0, mb, plan_ml, own_list != 0, SweepSwitches{unfused != 0, lpf8 != 0, no_tail != 0, false});
        printf("%s route=%d one=%d call_plan=%d lds_ok=%d ends=%d\n", nm, (int)R.route, (int)R.one, (int)R.call_plan, (int)R.lds_ok, (int)R.ends);
    }
    return 0;
}
