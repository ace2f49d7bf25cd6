# TEST INFRASTRUCTURE ONLY: libmpcqp_emu_c2d.so = the objects of libmpcqp_emu_kf_place.so (kf_place.mk) + the discretisation of
# continuous-time models (emu_c2d.cpp).  A makefile of its own: the other libraries stay WITHOUT that launcher.
include Makefile
libmpcqp_emu_c2d.so: $(STOCK_OBJS) $(EST_OBJS) emu_explicit.o emu_sim.o emu_est_init.o emu_kf_place.o emu_c2d.o
-include emu_explicit.d emu_sim.d emu_est_init.d emu_kf_place.d emu_c2d.d
