# TEST INFRASTRUCTURE ONLY: libmpcqp_emu_est_lds.so = libmpcqp_emu_est.so + the LDS-resident steady-state Riccati solve for
# 32 < max(nx, nym) <= 64 (emu_kf_dare_lds.cpp).  A makefile of its own: libmpcqp_emu_est.so stays the library WITHOUT that
# launcher, which refuses the steady solve beyond 32.
include Makefile
libmpcqp_emu_est_lds.so: $(STOCK_OBJS) $(EST_OBJS) emu_kf_dare_lds.o
-include emu_kf_dare_lds.d
