# TEST INFRASTRUCTURE ONLY: libmpcqp_emu_est_psd.so = libmpcqp_emu_est.so + the second pass of the steady-state Riccati
# solve (emu_kf_dare_psd.cpp).  A makefile of its own: libmpcqp_emu_est.so stays the library WITHOUT that launcher.
include Makefile
libmpcqp_emu_est_psd.so: $(STOCK_OBJS) $(EST_OBJS) emu_kf_dare_psd.o
-include emu_kf_dare_psd.d
